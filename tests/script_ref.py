"""Test oracle for zg_inputs_verify: a Python restatement of what verify_script
(script/src/interpreter.rs:288-360) does to a pay-to-pubkey-hash or pay-to-pubkey input under the flags the
acceptor passes (verification/src/accept_transaction.rs:334-358), plus a pure-Python RIPEMD-160 (hashlib has
none here). The signature hash is tests/sighash_ref.py, the ECDSA check tests/ecdsa_ref.py. Written from the
rules as the reference states them, independently of zebra_amd/csrc; pinned on the reference's own vectors
(tests/golden/inputs.json)."""
import hashlib

from tests import ecdsa_ref as E
from tests import sighash_ref as S

SCRIPT_HOST, SCRIPT_P2PKH, SCRIPT_P2PK = 0, 1, 2
DERSIG = 1
(INPUT_OK, INPUT_EQUALVERIFY, INPUT_SIGNATURE_DER, INPUT_EVAL_FALSE, INPUT_HOST, INPUT_TX_MALFORMED,
 INPUT_TX_NONCANONICAL, INPUT_RANGE) = range(8)
MAX_PUSH = 520
ZERO = b"\x00" * 32

# ---- RIPEMD-160 (Dobbertin, Bosselaers, Preneel 1996)
_RL = [list(range(16)), [7, 4, 13, 1, 10, 6, 15, 3, 12, 0, 9, 5, 2, 14, 11, 8],
       [3, 10, 14, 4, 9, 15, 8, 1, 2, 7, 0, 6, 13, 11, 5, 12], [1, 9, 11, 10, 0, 8, 12, 4, 13, 3, 7, 15, 14, 5, 6, 2],
       [4, 0, 5, 9, 7, 12, 2, 10, 14, 1, 3, 8, 11, 6, 15, 13]]
_RR = [[5, 14, 7, 0, 9, 2, 11, 4, 13, 6, 15, 8, 1, 10, 3, 12], [6, 11, 3, 7, 0, 13, 5, 10, 14, 15, 8, 12, 4, 9, 1, 2],
       [15, 5, 1, 3, 7, 14, 6, 9, 11, 8, 12, 2, 10, 0, 4, 13], [8, 6, 4, 1, 3, 11, 15, 0, 5, 12, 2, 13, 9, 7, 10, 14],
       [12, 15, 10, 4, 1, 5, 8, 7, 6, 2, 13, 14, 0, 3, 9, 11]]
_SL = [[11, 14, 15, 12, 5, 8, 7, 9, 11, 13, 14, 15, 6, 7, 9, 8], [7, 6, 8, 13, 11, 9, 7, 15, 7, 12, 15, 9, 11, 7, 13, 12],
       [11, 13, 6, 7, 14, 9, 13, 15, 14, 8, 13, 6, 5, 12, 7, 5], [11, 12, 14, 15, 14, 15, 9, 8, 9, 14, 5, 6, 8, 6, 5, 12],
       [9, 15, 5, 11, 6, 8, 13, 12, 5, 12, 13, 14, 11, 8, 5, 6]]
_SR = [[8, 9, 9, 11, 13, 15, 15, 5, 7, 7, 8, 11, 14, 14, 12, 6], [9, 13, 15, 7, 12, 8, 9, 11, 7, 7, 12, 7, 6, 15, 13, 11],
       [9, 7, 15, 11, 8, 6, 6, 14, 12, 13, 5, 14, 13, 13, 7, 5], [15, 5, 8, 11, 14, 14, 6, 14, 6, 9, 12, 9, 12, 5, 15, 8],
       [8, 5, 12, 9, 12, 5, 14, 6, 8, 13, 6, 5, 15, 13, 11, 11]]
_KL = [0x00000000, 0x5A827999, 0x6ED9EBA1, 0x8F1BBCDC, 0xA953FD4E]
_KR = [0x50A28BE6, 0x5C4DD124, 0x6D703EF3, 0x7A6D76E9, 0x00000000]
_M = 0xFFFFFFFF
_F = [lambda x, y, z: x ^ y ^ z, lambda x, y, z: (x & y) | (~x & _M & z), lambda x, y, z: (x | (~y & _M)) ^ z,
      lambda x, y, z: (x & z) | (y & ~z & _M), lambda x, y, z: x ^ (y | (~z & _M))]


def _rol(x, k):
    return ((x << k) | (x >> (32 - k))) & _M


def ripemd160(data):
    data = bytes(data)
    msg = data + b"\x80" + b"\x00" * ((55 - len(data)) % 64) + (8 * len(data)).to_bytes(8, "little")
    h = [0x67452301, 0xEFCDAB89, 0x98BADCFE, 0x10325476, 0xC3D2E1F0]
    for o in range(0, len(msg), 64):
        x = [int.from_bytes(msg[o + 4 * i:o + 4 * i + 4], "little") for i in range(16)]
        a, b, c, d, e = h
        a2, b2, c2, d2, e2 = h
        for g in range(5):
            for j in range(16):
                t = (_rol((a + _F[g](b, c, d) + x[_RL[g][j]] + _KL[g]) & _M, _SL[g][j]) + e) & _M
                a, e, d, c, b = e, d, _rol(c, 10), b, t
                t = (_rol((a2 + _F[4 - g](b2, c2, d2) + x[_RR[g][j]] + _KR[g]) & _M, _SR[g][j]) + e2) & _M
                a2, e2, d2, c2, b2 = e2, d2, _rol(c2, 10), b2, t
        h = [(h[1] + c + d2) & _M, (h[2] + d + e2) & _M, (h[3] + e + a2) & _M, (h[4] + a + b2) & _M, (h[0] + b + c2) & _M]
    return b"".join(v.to_bytes(4, "little") for v in h)


def dhash160(data):
    """crypto/src/lib.rs:202-206: RIPEMD-160 of SHA-256"""
    return ripemd160(hashlib.sha256(bytes(data)).digest())


# ---- the templates
def push(data, form=None):
    """the push instruction of `data`: the shortest form, or form 0x4c / 0x4d / 0x4e"""
    data = bytes(data)
    if form is None:
        form = len(data) if len(data) <= 0x4B else 0x4C if len(data) <= 0xFF else 0x4D
    if form <= 0x4B:
        assert form == len(data)
        return bytes([form]) + data
    return bytes([form]) + len(data).to_bytes({0x4C: 1, 0x4D: 2, 0x4E: 4}[form], "little") + data


def _push_at(s, o):
    """one push instruction at s[o:] -> (data offset, length, next offset), or None"""
    if o >= len(s):
        return None
    op, o = s[o], o + 1
    if op <= 0x4B:
        n = op
    elif op in (0x4C, 0x4D, 0x4E):
        w = {0x4C: 1, 0x4D: 2, 0x4E: 4}[op]
        if len(s) - o < w:
            return None
        n, o = int.from_bytes(s[o:o + w], "little"), o + w
    else:
        return None
    if n > MAX_PUSH or n > len(s) - o:
        return None
    return o, n, o + n


def classify(script_sig, script_pubkey):
    """-> (class, signature offset, length, key offset, length) as zg_script_class reports them"""
    sig, pk = bytes(script_sig), bytes(script_pubkey)
    host = (SCRIPT_HOST, 0, 0, 0, 0)
    if len(pk) == 25 and pk[:3] == b"\x76\xa9\x14" and pk[23:] == b"\x88\xac":
        a = _push_at(sig, 0)
        b = _push_at(sig, a[2]) if a else None
        if not b or b[2] != len(sig):
            return host
        return (SCRIPT_P2PKH, a[0], a[1], b[0], b[1])
    if (len(pk) == 35 and pk[0] == 0x21 or len(pk) == 67 and pk[0] == 0x41) and pk[-1] == 0xAC:
        a = _push_at(sig, 0)
        if not a or a[2] != len(sig):
            return host
        return (SCRIPT_P2PK, a[0], a[1], 1, len(pk) - 2)
    return host


def is_valid_signature_encoding(sig):
    """interpreter.rs:49-136; sig carries its hashtype byte"""
    n = len(sig)
    if n < 9 or n > 73 or sig[0] != 0x30 or sig[1] != n - 3:
        return False
    len_r = sig[3]
    if len_r + 5 >= n:
        return False
    len_s = sig[len_r + 5]
    if len_r + len_s + 7 != n:
        return False
    if sig[2] != 2 or len_r == 0 or sig[4] & 0x80:
        return False
    if len_r > 1 and sig[4] == 0 and not sig[5] & 0x80:
        return False
    if sig[len_r + 4] != 2 or len_s == 0 or sig[len_r + 6] & 0x80:
        return False
    if len_s > 1 and sig[len_r + 6] == 0 and not sig[len_r + 7] & 0x80:
        return False
    return True


def verify_input(raw, branch_id, index, script_pubkey, amount, flags):
    """what zg_inputs_verify reports for one item: (status, detail, hash)"""
    st, t = S.parse(raw)
    if st != S.TX_OK:
        return {S.TX_MALFORMED: INPUT_TX_MALFORMED, S.TX_NONCANONICAL: INPUT_TX_NONCANONICAL}[st], 0, ZERO
    if index >= len(t["inputs"]):
        return INPUT_RANGE, 0, ZERO
    script_sig, pk = bytes(t["inputs"][index]["script"]), bytes(script_pubkey)
    cls, so, sl, ko, kl = classify(script_sig, pk)
    if cls == SCRIPT_HOST:
        return INPUT_HOST, 0, ZERO
    sig = script_sig[so:so + sl]
    key = script_sig[ko:ko + kl] if cls == SCRIPT_P2PKH else pk[ko:ko + kl]
    if cls == SCRIPT_P2PKH and dhash160(key) != pk[3:23]:
        return INPUT_EQUALVERIFY, 0, ZERO
    if flags & DERSIG and sig and not is_valid_signature_encoding(sig):
        return INPUT_SIGNATURE_DER, 0, ZERO
    # check_signature (interpreter.rs:12-31): Public::from_slice takes any 33 or 65 bytes
    if len(key) not in (33, 65):
        return INPUT_EVAL_FALSE, E.verify(key, sig[:-1], ZERO), ZERO
    if not sig:
        return INPUT_EVAL_FALSE, E.verify(key, b"", ZERO), ZERO
    h = S.sighash_parsed(t, index, pk, amount, sig[-1], branch_id)
    ec = E.verify(key, sig[:-1], h)
    return (INPUT_EVAL_FALSE if ec else INPUT_OK), ec, h


def run(txs, branch_ids, items, flags):
    """the reference result of Context.inputs_verify(txs, branch_ids, items, flags)"""
    res = [verify_input(txs[t], branch_ids[t], i, pk, amt, flags) for t, i, pk, amt in items]
    return [S.parse(raw)[0] for raw in txs], [r[0] for r in res], [r[1] for r in res], [r[2] for r in res]
