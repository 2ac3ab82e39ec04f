"""Cases for the multisig tests (tests/test_multisig.py on the host build, tests/test_gpu_multisig.py on the GPU):
m-of-n OP_CHECKMULTISIG inputs, bare and behind pay-to-script-hash, as (txs, branch_ids, items, names) like
tests/script_cases.py. Signed here with the secrets of tests/golden/ecdsa.json through that module's Builder and
signed_push, over the three transaction formats; the reference's own 2-of-3 vector comes with its list. Expected
values always come from tests/multisig_ref.py."""
from tests import ecdsa_ref as E
from tests import multisig_ref as M
from tests import script_ref as R
from tests import sighash_ref as S
from tests.conftest import load_golden
from tests.script_cases import FORMATS, Builder, der_mutants, p2pk, p2pkh, reference_vectors

BIT = M.TEMPLATE_MULTISIG
push = R.push


def keys(count=18):
    out = []
    for v in load_golden("ecdsa.json")["signed"][:count]:
        d = int(v["secret"], 16)
        pt = E.mul(d, E.G)
        out.append((d, E.pubkey_bytes(pt, True), E.pubkey_bytes(pt, False)))
    return out


def ms_script(m, key_bytes, n=None):
    return bytes([0x50 + m]) + b"".join(push(k) for k in key_bytes) + bytes([0x50 + (len(key_bytes) if n is None else n)]) + b"\xae"


def p2sh(redeem):
    return b"\xa9\x14" + R.dhash160(redeem) + b"\x87"


class Cases(Builder):
    def __init__(self):
        super().__init__()
        self.keys = keys()

    def ms(self, name, t, index, m, ks, sigs, wrap=True, amount=700, dummy=b"\x00", form=None, script=None, item_script=None,
           tail=b"", **kw):
        """a spend of the m-of-len(ks) script over the keys numbered ks (negative: the uncompressed form of key -k-1).
        sigs, in push order: a key number (signs with hashtype 1), (key number, hashtype), or the push's bytes."""
        K = self.keys
        code = script if script is not None else ms_script(m, [K[k][1] if k >= 0 else K[-k - 1][2] for k in ks])

        def make(sign):
            out = dummy
            for s in sigs:
                if isinstance(s, (bytes, bytearray)):
                    out += push(s)
                elif callable(s):
                    out += push(s(sign))
                else:
                    k, ht = s if isinstance(s, tuple) else (s, 1)
                    out += push(sign(k if k >= 0 else -k - 1, ht))
            return out + (push(code, form) if wrap else b"") + tail
        # the script code a signer hashes is the script being evaluated: the redeem script, or the bare script
        self.spend(name, t, index, code, amount, make, item_script=item_script if item_script is not None else
                   (p2sh(code) if wrap else None), **kw)


def synthesized():
    b = Cases()
    K = b.keys
    # every (m, n) with n <= 4, behind P2SH at input 0 and bare at input 1 of one transaction; the signers spread
    # over the keys, compressed and uncompressed keys alternating
    j = 0
    for n in range(1, 5):
        for m in range(1, n + 1):
            for fmt in (FORMATS if n <= 3 else FORMATS[(m % 3):(m % 3) + 1]):
                t = b.tx(fmt, 2, 2, seed=1000 + j)
                ks = [(k if (k + j) % 2 else -k - 1) for k in range(n)]
                signers = sorted(((i * n) // m + (j % 2 if m < n else 0)) % n for i in range(m))
                assert len(set(signers)) == m
                b.ms("mn/p2sh/%d-of-%d/%s" % (m, n, fmt), t, 0, m, ks, [ks[i] for i in signers])
                b.ms("mn/bare/%d-of-%d/%s" % (m, n, fmt), t, 1, m, ks, [ks[i] for i in signers], wrap=False)
                j += 1
    # the widest scripts: sixteen uncompressed keys bare; fifteen compressed keys behind P2SH (513 bytes); sixteen
    # compressed keys are 547 bytes, no push instruction: HOST
    unc = [-k - 1 for k in range(16)]
    t = b.tx("sapling", 3, 1, seed=1100)
    b.ms("wide/1-of-16", t, 0, 1, unc, [unc[9]], wrap=False)
    b.ms("wide/8-of-16", t, 1, 8, unc, unc[1::2], wrap=False)
    b.ms("wide/16-of-16", t, 2, 16, unc, unc, wrap=False)
    t = b.tx("overwinter", 2, 1, seed=1101)
    b.ms("wide/15-of-15/p2sh", t, 0, 15, list(range(15)), list(range(15)))
    b.ms("host/16_keys_547_bytes", t, 1, 1, list(range(16)), [3])
    # 2-of-3: every signer subset, the signatures reversed, one signature twice, a signer that is not in the script
    j = 0
    for a in range(3):
        for c in range(3):
            t = b.tx(FORMATS[j % 3], 1, 1, seed=1200 + j)
            b.ms("2of3/%d%d" % (a, c), t, 0, 2, [0, -2, 2], [(0, -2, 2)[a], (0, -2, 2)[c]], wrap=bool(j % 2))
            j += 1
    t = b.tx("v2", 2, 1, seed=1220)
    b.ms("2of3/foreign_first", t, 0, 2, [0, 1, 2], [5, 2])
    b.ms("2of3/foreign_last", t, 1, 2, [0, 1, 2], [0, 5], wrap=False)
    # 2-of-5: the signers at each of the n - m + 1 offsets, and apart
    for j, pair in enumerate(((0, 1), (1, 2), (2, 3), (3, 4), (0, 4), (1, 3))):
        t = b.tx(FORMATS[j % 3], 1, 1, seed=1300 + j)
        b.ms("2of5/%d%d" % pair, t, 0, 2, [0, 1, -3, 3, 4], [(0, 1, -3, 3, 4)[i] for i in pair], wrap=j % 2 == 0)
    # a different hashtype per signature in one input
    for j, fmt in enumerate(FORMATS):
        t = b.tx(fmt, 2, 2, seed=1400 + j)
        b.ms("hashtypes/p2sh/%s" % fmt, t, 0, 3, [0, 1, 2], [(0, 1), (1, 0x82), (2, 3)])
        b.ms("hashtypes/bare/%s" % fmt, t, 1, 3, [3, 4, 5, 6], [(3, 0x83), (5, 2), (6, 0x81)], wrap=False)
    # encoding: a badly encoded push the walk reaches (SIGNATURE_DER under DERSIG, lax-parsed without it); one it never
    # reaches because an earlier pair already failed the walk; an empty push; a key with prefix 05
    t0 = b.tx("sapling", 1, 1, seed=1500)
    for j, name in enumerate(("r_padded", "s_padded", "total_length", "too_short", "r_negative", "not_compound")):
        t = b.tx(FORMATS[j % 3], 2, 1, seed=1501 + j)
        mutant = lambda sign, k, name=name: der_mutants(sign(k))[name]     # noqa: E731
        b.ms("der/reached_first/%s" % name, t, 0, 2, [0, 1, 2], [0, lambda sign, f=mutant: f(sign, 2)])
        b.ms("der/reached_second/%s" % name, t, 1, 2, [0, 1, 2], [lambda sign, f=mutant: f(sign, 0), 1], wrap=False)
    b.ms("der/never_reached", t0, 0, 2, [0, 1], [lambda sign: der_mutants(sign(0))["r_negative"], 5])
    t = b.tx("overwinter", 4, 1, seed=1520)
    b.ms("empty/one_of_two", t, 0, 2, [0, 1, 2], [b"", 2])
    b.ms("empty/only", t, 1, 1, [0, 1], [b""], wrap=False)
    b.ms("empty/hashtype_alone", t, 2, 1, [0], [b"\x01"])
    b.ms("empty/unreached", t, 3, 2, [0, 1], [b"", 5], wrap=False)
    t = b.tx("sapling", 3, 1, seed=1530)
    k05 = b"\x05" + K[7][1][1:]
    b.ms("key05/passes_on_the_next", t, 0, 1, None, [1], script=ms_script(1, [K[1][1], k05]))
    b.ms("key05/fails", t, 1, 1, None, [1], script=ms_script(1, [k05]), wrap=False)
    b.ms("key05/uncompressed_unreached", t, 2, 2, None, [1, 2],
         script=ms_script(2, [b"\x05" + K[7][2][1:], K[1][1], K[2][1]]))
    # a hash mismatch together with bad signatures: the mismatch wins, under either flag
    for j, pos in enumerate((2, 21)):
        t = b.tx(FORMATS[j], 1, 1, seed=1540 + j)
        code = ms_script(2, [K[0][1], K[1][1]])
        good = p2sh(code)
        b.ms("mismatch/%d" % pos, t, 0, 2, [0, 1], [lambda sign: der_mutants(sign(0))["r_negative"], 5],
             item_script=good[:pos] + bytes([good[pos] ^ 0x10]) + good[pos + 1:])
    t = b.tx("v2", 1, 1, seed=1545)
    good = p2sh(ms_script(1, [K[0][1]]))
    b.ms("mismatch/good_signature", t, 0, 1, [0], [0], item_script=good[:9] + bytes([good[9] ^ 1]) + good[10:])
    # the dummy is any push; the redeem push in every form
    t = b.tx("sapling", 2, 1, seed=1550)
    b.ms("dummy/01ff/p2sh", t, 0, 1, [0, 1], [1], dummy=b"\x01\xff")
    b.ms("dummy/pushdata1/bare", t, 1, 2, [0, 1], [0, 1], dummy=b"\x4c\x03abc", wrap=False)
    for j, form in enumerate((0x4C, 0x4D, 0x4E)):
        t = b.tx(FORMATS[j], 1, 1, seed=1560 + j)
        b.ms("redeem_push/%x" % form, t, 0, 1, [j], [j], form=form)
    # redeem scripts at SHA-256 padding edges: 375 bytes = 55 mod 64 (the padding just fits), 511 = 63 mod 64 (the
    # length spills into a further block); both over 252 bytes, so their compact size in the preimage is three bytes
    for j, (count, m) in enumerate(((9, 2), (13, 3))):
        t = b.tx(FORMATS[1 + j], 1, 1, seed=1570 + j)
        ks = list(range(count)) + [-count - 1]
        code = ms_script(m, [K[k][1] for k in range(count)] + [K[count][2]])
        assert len(code) == (375, 511)[j] and len(code) % 64 == (55, 63)[j]
        b.ms("padding/%d" % len(code), t, 0, m, ks, [ks[1], ks[-1]] if m == 2 else [ks[0], ks[6], ks[-1]])
    # near-misses, every one HOST
    t = b.tx("sapling", 18, 1, seed=1600)
    A, B = K[0][1], K[1][1]
    std = ms_script(1, [A, B])
    near = [("op_0_as_m", dict(script=b"\x00" + push(A) + b"\x51\xae", sigs=[])),
            ("counts_as_data_pushes", dict(script=b"\x01\x01" + push(A) + push(B) + b"\x01\x02\xae", sigs=[0])),
            ("checkmultisigverify", dict(script=std[:-1] + b"\xaf", sigs=[0])),
            ("one_signature_too_few", dict(script=ms_script(2, [A, B]), sigs=[0])),
            ("one_signature_too_many", dict(script=std, sigs=[0, 1])),
            ("missing_dummy", dict(script=std, sigs=[0], dummy=b"")),
            ("op_1_as_dummy", dict(script=std, sigs=[0], dummy=b"\x51")),
            ("op_16_as_signature", dict(script=std, sigs=[], dummy=b"\x00\x60")),
            ("op_1negate_as_dummy", dict(script=std, sigs=[0], dummy=b"\x4f")),
            ("redeem_is_p2pkh", dict(script=p2pkh(A), sigs=[0])),
            ("redeem_is_p2pk", dict(script=p2pk(A), sigs=[0])),
            ("trailing_byte_in_the_script", dict(script=std + b"\x00", sigs=[0])),
            ("m_above_n", dict(script=ms_script(2, [A]), sigs=[0, 0])),
            ("n_is_not_the_key_count", dict(script=ms_script(1, [A, B], n=3), sigs=[0])),
            ("key_push_of_32_bytes", dict(script=b"\x51\x20" + A[1:] + b"\x51\xae", sigs=[0])),
            ("key_push_past_the_end", dict(script=b"\x51\x21" + A[1:] + b"\x51\xae", sigs=[0]))]
    for j, (name, kw) in enumerate(near):
        b.ms("host/p2sh/" + name, t, j, 1, None, wrap=True, **kw)
    b.ms("host/p2sh/trailing_byte_in_script_sig", t, 16, 1, None, [0], script=std, tail=b"\x00")
    b.ms("host/p2sh/trailing_opcode_in_script_sig", t, 17, 1, None, [0], script=std, tail=b"\x61")
    t = b.tx("v2", 18, 1, seed=1601)
    for j, (name, kw) in enumerate(near):
        if not name.startswith("redeem_is_"):                        # (bare, those are the f15 templates themselves)
            b.ms("host/bare/" + name, t, j, 1, None, wrap=False, **kw)
    b.ms("host/bare/trailing_byte_in_script_sig", t, 16, 1, None, [0], script=std, tail=b"\x61", wrap=False)
    # a transaction mixing a P2PKH, a P2PK and two multisig inputs, of which one fails
    t = b.tx("sapling", 4, 2, seed=1700)
    b.spend("mixed/p2pkh", t, 0, p2pkh(K[0][1]), 11, lambda sign: push(sign(0)) + push(K[0][1]))
    b.ms("mixed/p2sh", t, 1, 2, [1, 2, 3], [1, 3], amount=12)
    b.spend("mixed/p2pk", t, 2, p2pk(K[4][2]), 13, lambda sign: push(sign(4, 0x81)))
    b.ms("mixed/bare_fails", t, 3, 2, [1, 2, 3], [3, 1], wrap=False, amount=14)
    # the same with every input passing, and RANGE on a multisig transaction
    t = b.tx("overwinter", 3, 1, seed=1701)
    b.spend("mixed_ok/p2pk", t, 0, p2pk(K[2][1]), 21, lambda sign: push(sign(2)))
    b.ms("mixed_ok/bare", t, 1, 1, [1, -3], [-3], wrap=False, amount=22)
    b.ms("mixed_ok/p2sh", t, 2, 3, [1, 2, 3], [1, 2, 3], amount=23)
    t = b.tx("v2", 1, 1, seed=1702)
    b.ms("range", t, 0, 1, [0], [0], item_index=1)
    return b.result()


_CACHE = {}


def case(flags):
    """(txs, branch_ids, items, names, reference result) of the synthesized list plus the reference's vectors, under
    `flags`; computed once"""
    if flags not in _CACHE:
        txs, br, items, names = synthesized()
        rt, rb, ri, _, _, rn = reference_vectors()
        items = items + [(t + len(txs), i, s, a) for t, i, s, a in ri]
        txs, br, names = txs + rt, br + rb, names + rn
        _CACHE[flags] = (txs, br, items, names, M.run(txs, br, items, flags))
    return _CACHE[flags]


def verdict_txs(flags):
    """the transactions of the case list whose every input is an item with a verdict -> [(raw, branch id,
    [(script_pubkey, amount) per input], the eval error the reference reports or None, the classes of its inputs)]"""
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
        cls = [M.match(tx["inputs"][i]["script"], ins[i][0], flags)[0] for i in sorted(ins)]
        out.append((txs[t], br[t], [ins[i][:2] for i in sorted(ins)],
                    ("Signature", bad[0], names[ins[bad[0]][2]]) if bad else None, cls))
    return out
