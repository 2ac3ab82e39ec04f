"""Test reference (CPU, hashlib): TransactionInputSigner::signature_hash (script/src/sign.rs:152-329) and the
statuses of the transaction parser (zg_tx_layout), restated independently of the library.

  * the Overwinter / Sapling branch is oracle.sapling_sig.sighash (sign.rs:249-329, already pinned by the
    reference's real Sapling transaction);
  * the Sprout branch (sign.rs:179-246: a double SHA-256 over a modified re-serialization) is restated here;
  * parse_status classifies a byte string as the reference's Transaction::deserialize does
    (chain/src/transaction.rs:249-330), plus the non-minimal compact sizes the reference reads and re-encodes.

Hashes are the 32 bytes of the reference's H256 (storage order)."""
import hashlib

from oracle import sapling_sig

TX_OK, TX_MALFORMED, TX_NONCANONICAL = 0, 1, 2
SIGHASH_OK, SIGHASH_TX_MALFORMED, SIGHASH_TX_NONCANONICAL, SIGHASH_INPUT_RANGE = 0, 1, 2, 3
OVERWINTER_VGID, SAPLING_VGID = 0x03C48270, 0x892F2085
ZERO = b"\x00" * 32

compact = sapling_sig.compact_bytes


class Malformed(Exception):
    pass


class _Rd:
    def __init__(self, d):
        self.d, self.o, self.noncanonical = bytes(d), 0, False

    def take(self, n):
        if n > len(self.d) - self.o:
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
        v = self.le({0xFD: 2, 0xFE: 4, 0xFF: 8}[b])
        if len(compact(v)) != {0xFD: 3, 0xFE: 5, 0xFF: 9}[b]:
            self.noncanonical = True
        return v

    def count(self, min_size):
        n = self.compact()
        if n * min_size > len(self.d) - self.o:
            raise Malformed("count")
        return n


def parse(raw):
    """-> (status, tx dict | None): the dict of oracle.sapling_sig.parse_tx_raw plus `scripts_in` and
    `sigver`; None when MALFORMED. For NONCANONICAL the dict holds the parsed values (what the reference
    would hash after re-encoding), not slices that could be hashed as they are."""
    rd = _Rd(raw)
    try:
        header = rd.le(4)
        ow, version = bool(header >> 31), header & 0x7FFFFFFF
        vgid = rd.le(4) if ow else 0
        is_ow = ow and version == 3 and vgid == OVERWINTER_VGID
        is_sap = ow and version == 4 and vgid == SAPLING_VGID
        if ow and not (is_ow or is_sap):
            raise Malformed("version")
        t = {"overwintered": ow, "version": version, "header": header, "vgid": vgid,
             "sigver": 0 if not ow else 2 if vgid == SAPLING_VGID else 1,
             "inputs": [], "outputs": [], "spends": [], "soutputs": [], "joinsplits": [], "js_pubkey": None}
        for _ in range(rd.count(41)):
            prev = rd.take(36)
            script = rd.take(rd.compact())
            t["inputs"].append({"prevout": prev, "script": script, "sequence": rd.take(4)})
        for _ in range(rd.count(9)):
            value = rd.take(8)
            script = rd.take(rd.compact())
            t["outputs"].append(value + compact(len(script)) + script)
        t["lock_time"] = rd.take(4)
        t["expiry"] = rd.take(4) if ow else b"\x00" * 4
        if is_sap:
            t["value_balance"] = rd.take(8)
            t["spends"] = [rd.take(384) for _ in range(rd.count(384))]
            t["soutputs"] = [rd.take(948) for _ in range(rd.count(948))]
        if version >= 2:
            size = 1698 if is_sap else 1802
            n = rd.count(size)
            t["joinsplits"] = [rd.take(size) for _ in range(n)]
            if n:
                t["js_pubkey"] = rd.take(32)
                t["js_sig"] = rd.take(64)
        if is_sap and (t["spends"] or t["soutputs"]):
            t["binding_sig"] = rd.take(64)
        if rd.o != len(rd.d):
            raise Malformed("trailing bytes")
    except Malformed:
        return TX_MALFORMED, None
    return (TX_NONCANONICAL if rd.noncanonical else TX_OK), t


def layout(raw):
    """what zg_tx_layout reports: (status, [header, inputs, outputs, joinsplits, spends, soutputs, sigver, len])"""
    st, t = parse(raw)
    if t is None:
        return st, [0] * 8
    return st, [t["header"], len(t["inputs"]), len(t["outputs"]), len(t["joinsplits"]), len(t["spends"]),
                len(t["soutputs"]), t["sigver"], len(raw)]


def _base(hashtype):
    return {2: 2, 3: 3}.get(hashtype & 0x1F, 1)   # 1 All, 2 None, 3 Single


def sprout(t, index, script, hashtype):
    """signature_hash_sprout (sign.rs:179-246)"""
    base, acp = _base(hashtype), bool(hashtype & 0x80)
    ins, outs = t["inputs"], t["outputs"]
    if index is None or index >= len(ins):
        if acp or base == 3:
            return ZERO
        index = (1 << 64) - 2
    script = bytes(script)
    if acp:
        new_in = [(ins[index]["prevout"], script, ins[index]["sequence"])]
    else:
        new_in = [(i["prevout"], script if n == index else b"",
                   b"\x00" * 4 if base in (2, 3) and n != index else i["sequence"]) for n, i in enumerate(ins)]
    if base == 1:
        new_out = list(outs)
    elif base == 3:
        new_out = [o if n == index else b"\xff" * 8 + b"\x00" for n, o in enumerate(outs[:index + 1])]
    else:
        new_out = []
    s = t["header"].to_bytes(4, "little") + compact(len(new_in))
    for prev, sc, seq in new_in:
        s += prev + compact(len(sc)) + sc + seq
    s += compact(len(new_out)) + b"".join(new_out) + t["lock_time"]
    if t["version"] >= 2:
        s += compact(len(t["joinsplits"]))
        if t["joinsplits"]:
            s += b"".join(t["joinsplits"]) + t["js_pubkey"] + b"\x00" * 64
    s += (hashtype & 0xFFFFFFFF).to_bytes(4, "little")
    return hashlib.sha256(hashlib.sha256(s).digest()).digest()


def sighash_parsed(t, index, script, amount, hashtype, branch_id):
    if t["sigver"] == 0:
        return sprout(t, index, script, hashtype)
    return sapling_sig.sighash(t, index, bytes(script), amount, hashtype & 0xFFFFFFFF, branch_id)


def sighash(raw, index, script, amount, hashtype, branch_id):
    """what zg_sighash returns for one item: (hash, status)"""
    st, t = parse(raw)
    if st != TX_OK:
        return ZERO, {TX_MALFORMED: SIGHASH_TX_MALFORMED, TX_NONCANONICAL: SIGHASH_TX_NONCANONICAL}[st]
    if t["sigver"] and index is not None and index >= len(t["inputs"]):
        return ZERO, SIGHASH_INPUT_RANGE
    return sighash_parsed(t, index, script, amount, hashtype, branch_id), SIGHASH_OK


def run(txs, branch_ids, items):
    """the reference result of Context.sighash(txs, branch_ids, items)"""
    tx_status = [parse(raw)[0] for raw in txs]
    res = [sighash(txs[tx], idx, sc, amt, ht, branch_ids[tx]) for tx, idx, sc, amt, ht in items]
    return tx_status, [r[0] for r in res], [r[1] for r in res]
