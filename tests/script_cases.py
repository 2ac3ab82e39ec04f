"""Cases for the template-input tests (tests/test_script.py on the host build, tests/test_gpu_script.py on the
GPU). A case list is (txs, branch_ids, items, flags), items as Context.inputs_verify takes them: (transaction
number, input index, the spent output's script_pubkey, its value). The reference's own vectors come from
tests/golden/inputs.json; the synthesized ones are signed here with the secrets of tests/golden/ecdsa.json over
tests/sighash_ref.py. Expected values always come from tests/script_ref.py."""
from tests import ecdsa_ref as E
from tests import script_ref as R
from tests import sighash_ref as S
from tests.conftest import load_golden
from tests.sighash_cases import OVERWINTER_BRANCH, SAPLING_BRANCH, long_form, make_tx

BRANCH = {"v1": 0, "v2": 0, "overwinter": OVERWINTER_BRANCH, "sapling": SAPLING_BRANCH}
FORMATS = ("v2", "overwinter", "sapling")
HASHTYPES = (1, 2, 3, 0x81, 0x82, 0x83, 0x50)      # All, None, Single, each with anyone-can-pay; one undefined byte
PREIMAGE_LENGTHS = (0, 1, 32, 33, 55, 56, 63, 64, 65, 119, 120, 520)


def secrets():
    """(secret, compressed key bytes, uncompressed key bytes) of the first keys of ecdsa.json"""
    out = []
    for v in load_golden("ecdsa.json")["signed"][:6]:
        d = int(v["secret"], 16)
        pt = E.mul(d, E.G)
        out.append((d, E.pubkey_bytes(pt, True), E.pubkey_bytes(pt, False)))
    return out


def p2pkh(key):
    return b"\x76\xa9\x14" + R.dhash160(key) + b"\x88\xac"


def p2pk(key):
    return bytes([len(key)]) + bytes(key) + b"\xac"


def set_script_sig(raw, index, script):
    """the transaction with input `index`'s script_sig replaced (canonical transactions only)"""
    st, t = S.parse(raw)
    assert st == S.TX_OK
    o = 4 + (4 if t["overwintered"] else 0) + len(S.compact(len(t["inputs"])))
    for i, inp in enumerate(t["inputs"]):
        old = len(S.compact(len(inp["script"]))) + len(inp["script"])
        if i == index:
            return raw[:o + 36] + S.compact(len(script)) + bytes(script) + raw[o + 36 + old:]
        o += 36 + old + 4
    raise IndexError(index)


def signed_push(raw, branch, index, script_pubkey, amount, d, hashtype):
    """the signature push content (DER || hashtype byte) of `d` over input `index`: the script_sig is no part of any
    signature hash, so a transaction is signed before its script_sigs are set"""
    h = S.sighash_parsed(S.parse(raw)[1], index, script_pubkey, amount, hashtype, branch)
    return E.der(*E.sign(d, h)) + bytes([hashtype])


class Builder:
    def __init__(self):
        self.txs, self.branches, self.items, self.names = [], [], [], []
        self.keys = secrets()

    def tx(self, fmt, n_in=2, n_out=2, seed=0, **kw):
        self.txs.append(make_tx(fmt, n_in, n_out, seed=seed, **kw))
        self.branches.append(BRANCH[fmt])
        return len(self.txs) - 1

    def spend(self, name, t, index, script_pubkey, amount, make_sig, item_amount=None, item_script=None, item_index=None):
        """make_sig(signature push content signed with hashtype ht by key k: sign(k, ht)) -> script_sig"""
        def sign(k, ht=1):
            return signed_push(self.txs[t], self.branches[t], index, script_pubkey, amount, self.keys[k][0], ht)
        self.txs[t] = set_script_sig(self.txs[t], index, make_sig(sign))
        self.items.append((t, index if item_index is None else item_index,
                           script_pubkey if item_script is None else item_script,
                           amount if item_amount is None else item_amount))
        self.names.append(name)

    def result(self):
        return self.txs, self.branches, self.items, self.names


def der_mutants(sig):
    """one signature push per failing branch of is_valid_signature_encoding, from a valid push (DER || hashtype);
    the lax parser still reads most of them"""
    s = bytearray(sig)
    lr = s[3]
    ls = s[lr + 5]
    out = {"too_short": bytes(s[:8]), "too_long": bytes(s[:-1]) + b"\x00" * (74 - len(s)) + bytes(s[-1:]),
           "not_compound": b"\x31" + bytes(s[1:]), "total_length": bytes(s[:1]) + bytes([s[1] + 1]) + bytes(s[2:]),
           "r_length_outside": bytes(s[:3]) + bytes([len(s) - 5]) + bytes(s[4:]),
           "lengths_do_not_add_up": bytes(s[:lr + 5]) + bytes([ls - 1]) + bytes(s[lr + 6:]),
           "r_not_integer": bytes(s[:2]) + b"\x03" + bytes(s[3:]),
           "s_not_integer": bytes(s[:lr + 4]) + b"\x03" + bytes(s[lr + 5:])}

    def rebuild(r, sb):
        body = b"\x02" + bytes([len(r)]) + r + b"\x02" + bytes([len(sb)]) + sb
        return b"\x30" + bytes([len(body)]) + body + bytes(s[-1:])
    r, sb = bytes(s[4:4 + lr]), bytes(s[lr + 6:lr + 6 + ls])
    out["r_empty"] = rebuild(b"", sb)
    out["r_negative"] = rebuild(bytes([r[0] | 0x80]) + r[1:], sb) if not r[0] & 0x80 else rebuild(r.lstrip(b"\x00"), sb)
    rs = r.lstrip(b"\x00")
    out["r_padded"] = rebuild(b"\x00" + bytes([rs[0] & 0x7F]) + rs[1:], sb)
    out["s_empty"] = rebuild(r, b"")
    out["s_negative"] = rebuild(r, bytes([sb[0] | 0x80]) + sb[1:])
    out["s_padded"] = rebuild(r, b"\x00" + bytes([sb[0] & 0x7F]) + sb[1:])
    for name, m in out.items():
        assert not R.is_valid_signature_encoding(m), name
    return out


def synthesized():
    """-> (txs, branch_ids, items, names); run with DERSIG on and off"""
    b = Builder()
    K = b.keys
    push = R.push

    # every format x every hashtype, P2PKH with a compressed key and P2PK with an uncompressed one
    for f, fmt in enumerate(FORMATS):
        for h, ht in enumerate(HASHTYPES):
            t = b.tx(fmt, 2, 2, seed=10 * f + h)
            k = (f + h) % len(K)
            b.spend("p2pkh/%s/%02x" % (fmt, ht), t, 0, p2pkh(K[k][1]), 5000 + h,
                    lambda sign, k=k, ht=ht: push(sign(k, ht)) + push(K[k][1]))
            b.spend("p2pk/%s/%02x" % (fmt, ht), t, 1, p2pk(K[k][2]), 7000 + h, lambda sign, k=k, ht=ht: push(sign(k, ht)))
    # compressed P2PK, uncompressed P2PKH
    t = b.tx("sapling", 2, 1, seed=40)
    b.spend("p2pk/compressed", t, 0, p2pk(K[0][1]), 1, lambda sign: push(sign(0)))
    b.spend("p2pkh/uncompressed", t, 1, p2pkh(K[1][2]), 2, lambda sign: push(sign(1)) + push(K[1][2]))
    # a transaction whose first input passes and whose second fails
    t = b.tx("overwinter", 2, 1, seed=45)
    b.spend("second_fails/0", t, 0, p2pkh(K[0][1]), 5, lambda sign: push(sign(0)) + push(K[0][1]))
    b.spend("second_fails/1", t, 1, p2pk(K[1][1]), 5, lambda sign: push(sign(2)))

    # key pushes as HASH160 preimages of every length, the matching hash in the script
    for n in PREIMAGE_LENGTHS:
        t = b.tx("overwinter" if n % 2 else "v2", 1, 1, seed=100 + n)
        pre = bytes((7 * i + n) & 0xFF for i in range(n))
        key = K[2][1] if n == 33 else K[2][2] if n == 65 else pre
        b.spend("preimage/%d" % n, t, 0, p2pkh(key), 9, lambda sign, key=key: push(sign(2)) + push(key))
    # one flipped hash byte, at either end of the 20 bytes
    for j, pos in enumerate((3, 12, 22, 15)):
        t = b.tx(FORMATS[j % 3], 1, 1, seed=200 + j)
        good = p2pkh(K[3][1])
        bad = good[:pos] + bytes([good[pos] ^ (1 << j)]) + good[pos + 1:]
        b.spend("equalverify/%d" % pos, t, 0, good, 3, lambda sign: push(sign(3)) + push(K[3][1]), item_script=bad)
    # an empty signature push; the hashtype byte alone; with a key that parses and one that does not
    for j, (sig, key) in enumerate(((b"", K[0][1]), (b"\x01", K[0][1]), (b"", b"\x05" * 33), (b"\x01", b"\x02" + b"\xff" * 32),
                                    (b"", K[1][2]), (b"\x83", K[1][2]))):
        t = b.tx(FORMATS[j % 3], 2, 2, seed=300 + j)
        b.spend("empty_sig/p2pkh/%d" % j, t, 0, p2pkh(key), 4, lambda sign, sig=sig, key=key: push(sig) + push(key))
        b.spend("empty_sig/p2pk/%d" % j, t, 1, p2pk(key), 4, lambda sign, sig=sig: push(sig))
    # each branch of is_valid_signature_encoding failed once
    t0 = b.tx("sapling", 1, 1, seed=400)
    proto = signed_push(b.txs[t0], SAPLING_BRANCH, 0, p2pkh(K[4][1]), 11, K[4][0], 1)
    for j, (name, m) in enumerate(sorted(der_mutants(proto).items())):
        t = b.tx(FORMATS[j % 3], 1, 1, seed=401 + j)
        if j % 2:
            b.spend("der/%s" % name, t, 0, p2pkh(K[4][1]), 11, lambda sign, m=m: push(m) + push(K[4][1]))
        else:
            b.spend("der/%s" % name, t, 0, p2pk(K[4][1]), 11, lambda sign, m=m: push(m))
    b.spend("der/valid", t0, 0, p2pkh(K[4][1]), 11, lambda sign: push(proto) + push(K[4][1]))
    # a good encoding over the wrong message: bad signatures (ZG_ECDSA_SIGNATURE), a key that is not on the curve
    for j in range(4):
        t = b.tx(FORMATS[j % 3], 2, 1, seed=500 + j)
        b.spend("wrong_key/%d" % j, t, 0, p2pk(K[j][1]), 6, lambda sign, j=j: push(sign(j + 1)))
        offcurve = b"\x04" + K[j][2][1:64] + bytes([K[j][2][64] ^ 1])
        b.spend("off_curve/%d" % j, t, 1, p2pkh(offcurve), 6, lambda sign, j=j, oc=offcurve: push(sign(j)) + push(oc))
    # the wrong amount: an overwintered transaction fails, a Sprout one never hashes it
    for j, fmt in enumerate(("overwinter", "sapling", "v2", "v1")):
        t = b.tx(fmt, 1, 2, seed=600 + j)
        b.spend("wrong_amount/%s" % fmt, t, 0, p2pkh(K[5][1]), 1000, lambda sign: push(sign(5)) + push(K[5][1]), item_amount=1001)
    # template near-misses, every one HOST
    t = b.tx("sapling", 9, 1, seed=700)
    good = p2pkh(K[0][1])
    both = lambda sign: push(sign(0)) + push(K[0][1])   # noqa: E731
    b.spend("host/24_bytes", t, 0, good, 1, both, item_script=good[:-1])
    b.spend("host/26_bytes", t, 1, good, 1, both, item_script=good + b"\xac")
    b.spend("host/equal_not_equalverify", t, 2, good, 1, both, item_script=good[:23] + b"\x87" + good[24:])
    b.spend("host/p2pk_32_byte_key", t, 3, p2pk(K[0][1]), 1, lambda sign: push(sign(0)), item_script=b"\x20" + K[0][1][1:] + b"\xac")
    b.spend("host/third_push", t, 4, good, 1, lambda sign: push(b"") + push(sign(0)) + push(K[0][1]))
    b.spend("host/op_1", t, 5, p2pk(K[0][1]), 1, lambda sign: b"\x51")
    b.spend("host/pushdata1_past_end", t, 6, p2pk(K[0][1]), 1, lambda sign: b"\x4c\x49" + sign(0))
    b.spend("host/521_byte_push", t, 7, good, 1, lambda sign: push(sign(0)) + b"\x4d\x09\x02" + b"\x00" * 521)
    b.spend("host/p2pkh_one_push", t, 8, good, 1, lambda sign: push(sign(0)))
    # PUSHDATA1 / 2 / 4 forms of a valid spend
    for j, form in enumerate((0x4C, 0x4D, 0x4E)):
        t = b.tx(FORMATS[j], 2, 1, seed=800 + j)
        b.spend("pushdata/p2pkh/%x" % form, t, 0, p2pkh(K[1][1]), 8,
                lambda sign, form=form: push(sign(1), form) + push(K[1][1], form))
        b.spend("pushdata/p2pk/%x" % form, t, 1, p2pk(K[1][2]), 8, lambda sign, form=form: push(sign(1, 0x82), form))
    # RANGE for every format; malformed and non-canonical transactions
    for j, fmt in enumerate(("v1", "v2", "overwinter", "sapling")):
        t = b.tx(fmt, 1, 1, seed=900 + j)
        b.spend("range/%s" % fmt, t, 0, p2pkh(K[2][1]), 1, lambda sign: push(sign(2)) + push(K[2][1]),
                item_index=(1, 2, 1000, 0xFFFFFFFF)[j])
    for j, fmt in enumerate(FORMATS + ("v1",)):
        t = b.tx(fmt, 1, 1, seed=950 + j)
        b.spend("malformed/%s" % fmt, t, 0, p2pkh(K[2][1]), 1, lambda sign: push(sign(2)) + push(K[2][1]))
        b.txs[t] = b.txs[t][:-1]
        b.txs.append(make_tx(fmt, 2, 2, seed=960 + j, enc={"out_script": long_form(0xFD)}))
        b.branches.append(BRANCH[fmt])
        b.items.append((len(b.txs) - 1, 0, p2pkh(K[2][1]), 1))
        b.names.append("noncanonical/%s" % fmt)
    return b.result()


def reference_vectors():
    """the reference's own transactions (tests/golden/inputs.json) -> (txs, branch_ids, items, flags per item,
    expected status per item, names)"""
    g = load_golden("inputs.json")
    txs, br, items, flags, want, names = [], [], [], [], [], []
    for v in g["vectors"]:
        txs.append(bytes.fromhex(v["tx"]))
        br.append(v["branch_id"])
        items.append((len(txs) - 1, v["input_index"], bytes.fromhex(v["script_pubkey"]), v["amount"]))
        flags.append(v["flags"])
        want.append(v["status"])
        names.append(v["name"])
    return txs, br, items, flags, want, names


_CACHE = {}


def case(flags):
    """(txs, branch_ids, items, names, reference result) of the synthesized list plus the reference's vectors, under
    `flags`; computed once"""
    if flags not in _CACHE:
        txs, br, items, names = synthesized()
        rt, rb, ri, _, _, rn = reference_vectors()
        items = items + [(t + len(txs), i, s, a) for t, i, s, a in ri]
        txs, br, names = txs + rt, br + rb, names + rn
        _CACHE[flags] = (txs, br, items, names, R.run(txs, br, items, flags))
    return _CACHE[flags]


def template_txs(flags):
    """the transactions of the case list whose every input is an item with a verdict (a template, in range, the
    transaction parsed) -> [(raw, branch id, [(script_pubkey, amount) per input], the eval error the reference
    reports: ("Signature", lowest failing input, name) or None)]"""
    txs, br, items, _, (_, st, _, _) = case(flags)
    names = {R.INPUT_EQUALVERIFY: "EqualVerify", R.INPUT_SIGNATURE_DER: "SignatureDer", R.INPUT_EVAL_FALSE: "EvalFalse"}
    by = {}
    for (t, i, pk, amount), s in zip(items, st):
        by.setdefault(t, {})[i] = (pk, amount, s)
    out = []
    for t, ins in sorted(by.items()):
        pst, tx = S.parse(txs[t])
        if pst != S.TX_OK or sorted(ins) != list(range(len(tx["inputs"]))) or any(v[2] > R.INPUT_EVAL_FALSE for v in ins.values()):
            continue
        bad = [i for i in sorted(ins) if ins[i][2] != R.INPUT_OK]
        out.append((txs[t], br[t], [ins[i][:2] for i in sorted(ins)],
                    ("Signature", bad[0], names[ins[bad[0]][2]]) if bad else None))
    return out
