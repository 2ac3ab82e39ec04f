"""Test oracle for zg_inputs_verify's multisig classes: tests/script_ref.py plus a Python
restatement of what verify_script (script/src/interpreter.rs:228-286) does to an m-of-n OP_CHECKMULTISIG input, bare
or behind pay-to-script-hash, under the flags the acceptor passes (verification/src/accept_transaction.rs:334-358):
the template matcher as include/zg.h states it and OP_CHECKMULTISIG's walk (interpreter.rs:786-840). Written from the
rules, independently of zebra_amd/csrc; pinned on the reference's own vector, test_check_transaction_multisig
(tests/golden/inputs.json). With the opt-in bit clear it is script_ref."""
from tests import ecdsa_ref as E
from tests import script_ref as R
from tests import sighash_ref as S

SCRIPT_MULTISIG, SCRIPT_P2SH_MULTISIG = 3, 4
TEMPLATE_MULTISIG = 0x100
ZERO = R.ZERO


def multisig_form(s):
    """s = OP_m <key>...<key> OP_n ae -> (m, n, [(key offset, length)] in push order), or None"""
    s = bytes(s)
    if len(s) < 3 or not 0x51 <= s[0] <= 0x60:
        return None
    o, keys = 1, []
    while o < len(s) and s[o] in (0x21, 0x41):
        if o + 1 + s[o] > len(s):
            return None
        keys.append((o + 1, s[o]))
        o += 1 + s[o]
    if len(s) - o != 2 or not 0x51 <= s[o] <= 0x60 or s[o + 1] != 0xAE:
        return None
    m, n = s[0] - 0x50, s[o] - 0x50
    return (m, n, keys) if n == len(keys) and m <= n else None


def pushes(s):
    """every instruction of s a push -> [(data offset, length, instruction offset)], else None"""
    out, o = [], 0
    while o < len(s):
        p = R._push_at(s, o)
        if not p:
            return None
        out.append((p[0], p[1], o))
        o = p[2]
    return out


def match(script_sig, script_pubkey, flags):
    """what zg_script_match reports: (class, m, n, redeem offset, redeem length, pairs, first signature push, 0)"""
    sig, pk = bytes(script_sig), bytes(script_pubkey)
    cls = R.classify(sig, pk)[0]
    if cls:
        return (cls, 1, 1, 0, 0, 1, 0, 0)
    host = (0,) * 8
    if not flags & TEMPLATE_MULTISIG:
        return host
    p2sh = len(pk) == 23 and pk[:2] == b"\xa9\x14" and pk[22] == 0x87
    form = None if p2sh else multisig_form(pk)
    if not p2sh and not form:
        return host
    ps = pushes(sig)
    if ps is None:
        return host
    red = (0, 0)
    if p2sh:
        if len(ps) < 3:
            return host
        red = ps.pop()[:2]
        form = multisig_form(sig[red[0]:red[0] + red[1]])
        if not form:
            return host
    m, n, _ = form
    if len(ps) != m + 1:
        return host
    return (SCRIPT_P2SH_MULTISIG if p2sh else SCRIPT_MULTISIG, m, n, red[0], red[1], m * (n - m + 1), ps[1][2], 0)


def walk(sigs, keys, check, dersig):
    """OP_CHECKMULTISIG's loop (interpreter.rs:803-821) over signatures and keys in pop order. check(s, k) -> the
    ECDSA_* status of the pair -> (status, detail, (s, k) of the last pair checked or None)"""
    s = k = 0
    success, last, ec = True, None, 0
    while s < len(sigs) and success:
        if dersig and sigs[s] and not R.is_valid_signature_encoding(sigs[s]):
            return R.INPUT_SIGNATURE_DER, 0, None
        last, ec = (s, k), check(s, k)
        if ec == 0:
            s += 1
        k += 1
        success = len(sigs) - s <= len(keys) - k
    return (R.INPUT_OK, 0, last) if success else (R.INPUT_EVAL_FALSE, ec, last)


def verify_input(raw, branch_id, index, script_pubkey, amount, flags):
    """what zg_inputs_verify reports for one item: (status, detail, hash)"""
    base = R.verify_input(raw, branch_id, index, script_pubkey, amount, flags & R.DERSIG)
    if base[0] != R.INPUT_HOST or not flags & TEMPLATE_MULTISIG:
        return base
    t = S.parse(raw)[1]
    sig, pk = bytes(t["inputs"][index]["script"]), bytes(script_pubkey)
    mt = match(sig, pk, flags)
    if not mt[0]:
        return base
    code = sig[mt[3]:mt[3] + mt[4]] if mt[0] == SCRIPT_P2SH_MULTISIG else pk
    if mt[0] == SCRIPT_P2SH_MULTISIG and R.dhash160(code) != pk[2:22]:
        return R.INPUT_EVAL_FALSE, 0, ZERO
    m, n, key_at = multisig_form(code)
    keys = [code[o:o + l] for o, l in key_at][::-1]                  # pop order: the last pushed first
    sigs = [sig[o:o + l] for o, l, _ in pushes(sig)[1:1 + m]][::-1]
    hashes = {}

    def check(s, k):
        if not sigs[s]:                                              # check_signature: false, no hash computed
            hashes[(s, k)] = ZERO
            return E.verify(keys[k], b"", ZERO)
        h = hashes[(s, k)] = S.sighash_parsed(t, index, code, amount, sigs[s][-1], branch_id)
        return E.verify(keys[k], sigs[s][:-1], h)
    st, dt, last = walk(sigs, keys, check, flags & R.DERSIG)
    return st, dt, hashes[last] if last else ZERO


def run(txs, branch_ids, items, flags):
    """the reference result of Context.inputs_verify(txs, branch_ids, items, flags)"""
    res = [verify_input(txs[t], branch_ids[t], i, pk, amt, flags) for t, i, pk, amt in items]
    return [S.parse(raw)[0] for raw in txs], [r[0] for r in res], [r[1] for r in res], [r[2] for r in res]
