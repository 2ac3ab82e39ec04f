#!/usr/bin/env python3
"""Generate tests/golden/ecdsa.json: the fixtures of the secp256k1 ECDSA check (zg_ecdsa_verify).

Reads the reference as TEXT only, the way gen_golden.py does: the key-pair vectors of
keys/src/keypair.rs:96-105 (checked there at :173-181) and the five legacy-sighash transactions of
script/src/interpreter.rs:1817-1907; public keys are derived from the WIF secrets, sighashes with
signature_hash_sprout (SIGHASH_ALL, script code as the issue of each vector says). Every expected
status comes from tests/ecdsa_ref.py; each named edge case has the status listed in EDGE_STATUS and
every status 0-3 occurs at least 8 times among the edges.

    python tests/golden/gen_ecdsa.py
"""
import json
import os
import random
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

import ecdsa_ref as E  # noqa: E402

OKS, PUB, ENC, SIG = E.OK, E.PUBLIC, E.SIGNATURE_ENCODING, E.SIGNATURE
EDGE_STATUS = dict(
    [("key_len_%d" % k, PUB) for k in (0, 32, 34, 64, 66)] +
    [("key33_prefix04", PUB), ("key65_prefix02", PUB), ("key_x_no_root", PUB), ("key_off_curve", PUB),
     ("key_x_plus_p_compressed", PUB), ("key_x_plus_p_uncompressed", PUB), ("key_hybrid_right_parity", OKS),
     ("key_hybrid_wrong_parity", PUB), ("key_hybrid_compressed_source", OKS), ("key_parity_swapped", SIG),
     ("sig_empty", ENC), ("sig_wrong_first_byte", ENC)] +
    [("sig_truncated_%d" % k, ENC) for k in range(1, 9)] +
    [("sig_seq_long_form_wrong_value", OKS), ("sig_r_long_form", OKS), ("sig_r_long_form_zero_length_bytes", OKS),
     ("sig_s_length_past_end", ENC), ("sig_8_length_bytes", ENC), ("sig_trailing_bytes", OKS),
     ("sig_top_bit_unpadded", OKS), ("sig_r_33_significant_bytes", SIG), ("sig_r_eq_n", SIG), ("sig_r_zero", SIG),
     ("sig_r_empty_integer", SIG), ("sig_s_zero", SIG), ("sig_s_eq_n", SIG),
     ("arith_x_ge_n_second_compare", OKS), ("arith_r_plus_n_ge_p", SIG), ("arith_q_eq_g_doubling", OKS),
     ("arith_q_eq_neg_g_infinity", SIG), ("arith_u1g_eq_u2q", OKS), ("arith_m_plus_rd_zero_infinity", SIG),
     ("arith_zero_message", OKS), ("arith_message_ge_n", OKS), ("msg_flip", SIG)])


def pushes(script):
    """the data pushes of a script (OP_0, direct pushes, OP_PUSHDATA1); other opcodes are skipped"""
    out, o = [], 0
    while o < len(script):
        op = script[o]
        o += 1
        if op == 0x4c:
            op = script[o]
            o += 1
        elif op > 75:
            continue
        out.append(script[o:o + op])
        o += op
    return out


def reference_text():
    from gen_golden import REF
    return (open(os.path.join(REF, "keys", "src", "keypair.rs")).read(),
            open(os.path.join(REF, "script", "src", "interpreter.rs")).read())


def real_entries():
    keypair, interp = reference_text()
    const = dict(re.findall(r'const (\w+): &\'static str = "(\w+)";', keypair))
    out = []
    very = E.dhash256(b"Very deterministic message")
    empty = E.dhash256(b"")
    for sec, sg in (("SECRET_1", "SIGN_1"), ("SECRET_1C", "SIGN_1"), ("SECRET_2", "SIGN_2"), ("SECRET_2C", "SIGN_2")):
        d, comp = E.wif_secret(const[sec])
        assert comp == sec.endswith("C")
        pk = E.pubkey_bytes(E.mul(d, E.G), comp)
        out.append(("keypair_%s_%s" % (sec.lower(), sg.lower()), pk, bytes.fromhex(const[sg]), very, OKS))
    for sec, sg in (("SECRET_2C", "SIGN_2"), ("SECRET_1", "SIGN_1")):   # keypair.rs:180 and its SIGN_1 twin
        d, comp = E.wif_secret(const[sec])
        out.append(("keypair_%s_empty_message" % sec.lower(), E.pubkey_bytes(E.mul(d, E.G), comp),
                    bytes.fromhex(const[sg]), empty, SIG))

    def vector(fn):
        body = interp[interp.index("fn %s()" % fn):]
        body = body[:body.index("\n\t}\n")]
        tx = bytes.fromhex(re.search(r'let tx: Transaction = "(\w+)"', body).group(1))
        inp = bytes.fromhex(re.search(r'let input: Script = "(\w+)"', body).group(1))
        outp = bytes.fromhex(re.search(r'let output: Script = "(\w+)"', body).group(1))
        return tx, inp, outp, E.dhash256(tx)[::-1].hex()

    def strip(sig):
        assert sig[-1] == 1   # SIGHASH_ALL
        return sig[:-1]

    tx, inp, outp, txid = vector("test_check_transaction_signature")
    assert txid.startswith("3f285f08")
    sg, pk = pushes(inp)
    out.append(("p2pkh_" + txid[:8], pk, strip(sg), E.legacy_sighash_all(tx, 0, outp), OKS))
    tx, inp, outp, txid = vector("test_transaction_with_high_s_signature")
    assert txid.startswith("12b5633b")
    (sg,), (pk,) = pushes(inp), pushes(outp)
    assert E.parse_der_lax(strip(sg))[1] > E.N // 2
    out.append(("p2pk_high_s_" + txid[:8], pk, strip(sg), E.legacy_sighash_all(tx, 0, outp), OKS))
    tx, inp, outp, txid = vector("test_transaction_from_124276")
    assert txid.startswith("fb0a1d8d")
    sg, pk = pushes(inp)
    assert strip(sg)[:5].hex() == "3048022200"   # not strict DER
    out.append(("lax_der_" + txid[:8], pk, strip(sg), E.legacy_sighash_all(tx, 0, outp), OKS))
    tx, inp, outp, txid = vector("test_check_transaction_multisig")
    assert tx[5:37][::-1].hex().startswith("02b08211")   # the reference names this vector by the output it spends
    txid = "02b08211"
    _, s1, s2, redeem = pushes(inp)
    keys = pushes(redeem)
    assert len(keys) == 3
    m = E.legacy_sighash_all(tx, 0, redeem)
    for j, sg in enumerate((s1, s2)):
        good = [k for k in range(3) if E.verify(keys[k], strip(sg), m) == OKS]
        assert len(good) == 1
        out.append(("multisig_%s_sig%d_key%d" % (txid[:8], j, good[0]), keys[good[0]], strip(sg), m, OKS))
        other = (good[0] + 1) % 3
        out.append(("multisig_%s_sig%d_key%d_mismatch" % (txid[:8], j, other), keys[other], strip(sg), m, SIG))
    tx, inp, outp, txid = vector("test_arithmetic_correct_arguments_order")
    assert txid.startswith("54fabd73")
    sg = pushes(inp)[0]
    pk = [p for p in pushes(outp) if len(p) == 33][0]
    out.append(("compressed_key_" + txid[:8], pk, strip(sg), E.legacy_sighash_all(tx, 0, outp), OKS))
    for name, pk, sg, m, st in out:
        assert E.verify(pk, sg, m) == st, name
    return [{"name": n, "pubkey": pk.hex(), "sig": sg.hex(), "sighash": m.hex(), "status": st}
            for n, pk, sg, m, st in out]


def b32(v):
    return v.to_bytes(32, "big")


def main():
    rnd = random.Random(256)
    real = real_entries()

    signed = []
    for i in range(64):
        d, msg = rnd.randrange(1, E.N), rnd.randbytes(32)
        r, s = E.sign(d, msg)
        if i % 4 == 3:
            s = E.N - s
        pk = E.pubkey_bytes(E.mul(d, E.G), i % 2 == 0)
        signed.append({"secret": b32(d).hex(), "pubkey": pk.hex(), "sig": E.der(r, s).hex(), "msg": msg.hex()})
        assert E.verify(pk, E.der(r, s), msg) == OKS

    edges = {}

    def edge(name, pk, sg, m):
        assert name not in edges
        edges[name] = (bytes(pk), bytes(sg), bytes(m))

    d0 = rnd.randrange(1, E.N)
    q0 = E.mul(d0, E.G)
    m0 = rnd.randbytes(32)
    r0, s0 = E.sign(d0, m0)
    pk0, pk0c, sg0 = E.pubkey_bytes(q0, False), E.pubkey_bytes(q0, True), E.der(r0, s0)
    assert len(sg0) >= 70

    # ---- keys
    for k in (0, 32, 34, 64, 66):
        edge("key_len_%d" % k, (pk0 + b"\x00")[:k], sg0, m0)
    edge("key33_prefix04", b"\x04" + pk0c[1:], sg0, m0)
    edge("key65_prefix02", b"\x02" + pk0[1:], sg0, m0)
    x = 1
    while E.lift_x(x, 0) is not None:
        x += 1
    edge("key_x_no_root", b"\x02" + b32(x), sg0, m0)
    edge("key_off_curve", pk0[:64] + bytes([pk0[64] ^ 1]), sg0, m0)
    x = 1
    while E.lift_x(x, 0) is None:
        x += 1
    assert x + E.P < 2 ** 256
    small = E.lift_x(x, 0)
    edge("key_x_plus_p_compressed", b"\x02" + b32(x + E.P), sg0, m0)
    edge("key_x_plus_p_uncompressed", b"\x04" + b32(x + E.P) + b32(small[1]), sg0, m0)
    edge("key_hybrid_right_parity", bytes([6 | (q0[1] & 1)]) + pk0[1:], sg0, m0)
    edge("key_hybrid_wrong_parity", bytes([7 ^ (q0[1] & 1)]) + pk0[1:], sg0, m0)
    d1 = rnd.randrange(1, E.N)
    q1 = E.mul(d1, E.G)
    m1 = rnd.randbytes(32)
    edge("key_hybrid_compressed_source", bytes([6 | (q1[1] & 1)]) + E.pubkey_bytes(q1, False)[1:],
         E.der(*E.sign(d1, m1)), m1)
    edge("key_parity_swapped", bytes([pk0c[0] ^ 1]) + pk0c[1:], sg0, m0)

    # ---- signature encodings
    def integer(v, raw=None):
        b = raw if raw is not None else E.der(v, 1)[2:-3][2:]
        return b"\x02" + bytes([len(b)]) + b

    def seq(body):
        return b"\x30" + bytes([len(body)]) + body

    rb = E.der(r0, s0)[2:]
    rb, sb = rb[2:2 + rb[1]], rb[2 + rb[1]:][2:]
    edge("sig_empty", pk0, b"", m0)
    edge("sig_wrong_first_byte", pk0, b"\x31" + sg0[1:], m0)
    for k in range(1, 9):
        edge("sig_truncated_%d" % k, pk0, sg0[:k], m0)
    edge("sig_seq_long_form_wrong_value", pk0, b"\x30\x81\x05" + sg0[2:], m0)
    edge("sig_r_long_form", pk0, seq(b"\x02\x81" + bytes([len(rb)]) + rb + integer(0, sb)), m0)
    edge("sig_r_long_form_zero_length_bytes", pk0, seq(b"\x02\x83\x00\x00" + bytes([len(rb)]) + rb + integer(0, sb)), m0)
    edge("sig_s_length_past_end", pk0, seq(integer(0, rb) + b"\x02" + bytes([len(sb) + 1]) + sb), m0)
    edge("sig_8_length_bytes", pk0, seq(b"\x02\x88\x01" + bytes(6) + bytes([len(rb)]) + rb + integer(0, sb)), m0)
    edge("sig_trailing_bytes", pk0, sg0 + b"\x01\xff\x30", m0)
    while True:
        mt = rnd.randbytes(32)
        rt, st = E.sign(d0, mt)
        if rt >> 255:
            break
    edge("sig_top_bit_unpadded", pk0, seq(integer(0, b32(rt)) + integer(st)), mt)
    edge("sig_r_33_significant_bytes", pk0, seq(integer(0, b"\x01" + b32(r0)) + integer(0, sb)), m0)
    edge("sig_r_eq_n", pk0, E.der(E.N, s0), m0)
    edge("sig_r_zero", pk0, E.der(0, s0), m0)
    edge("sig_r_empty_integer", pk0, seq(b"\x02\x00" + integer(0, sb)), m0)
    edge("sig_s_zero", pk0, E.der(r0, 0), m0)
    edge("sig_s_eq_n", pk0, E.der(r0, E.N), m0)

    # ---- arithmetic, constructed without discrete logs: R = [u1] G + [u2] Q, s = r / u2, m = u1 s
    def constructed(name, rp, r, u1, u2):
        q = E.mul(pow(u2, -1, E.N), E.add(rp, E.neg(E.mul(u1, E.G))))
        s = r * pow(u2, -1, E.N) % E.N
        edge(name, E.pubkey_bytes(q, rnd.random() < 0.5), E.der(r, s), b32(u1 * s % E.N))

    x = E.N + 1
    while E.lift_x(x, 0) is None:
        x += 1
    assert x < E.P
    constructed("arith_x_ge_n_second_compare", E.lift_x(x, 1), x - E.N, rnd.randrange(1, E.N), rnd.randrange(1, E.N))
    # x(R') = small, r = small + p - n: r + n = small (mod p), but r + n >= p and the compare is not made
    constructed("arith_r_plus_n_ge_p", small, small[0] + E.P - E.N, rnd.randrange(1, E.N), rnd.randrange(1, E.N))
    u = rnd.randrange(1, E.N)
    r = E.mul(2 * u, E.G)[0] % E.N
    s = r * pow(u, -1, E.N) % E.N
    edge("arith_q_eq_g_doubling", E.pubkey_bytes(E.G, True), E.der(r, s), b32(u * s % E.N))
    edge("arith_q_eq_neg_g_infinity", E.pubkey_bytes(E.neg(E.G), False), E.der(r, s), b32(u * s % E.N))
    d, u2 = rnd.randrange(1, E.N), rnd.randrange(1, E.N)
    u1 = u2 * d % E.N
    r = E.mul(2 * u1, E.G)[0] % E.N
    s = r * pow(u2, -1, E.N) % E.N
    edge("arith_u1g_eq_u2q", E.pubkey_bytes(E.mul(d, E.G), False), E.der(r, s), b32(u1 * s % E.N))
    r, s = rnd.randrange(1, E.N), rnd.randrange(1, E.N)
    edge("arith_m_plus_rd_zero_infinity", E.pubkey_bytes(E.mul(d, E.G), True), E.der(r, s), b32(-r * d % E.N))
    k = rnd.randrange(1, E.N)
    r = E.mul(k, E.G)[0] % E.N
    s = r * d * pow(k, -1, E.N) % E.N
    edge("arith_zero_message", E.pubkey_bytes(E.mul(d, E.G), True), E.der(r, s), bytes(32))
    ms = rnd.randrange(2 ** 256 - E.N)
    edge("arith_message_ge_n", pk0, E.der(*E.sign(d0, b32(ms))), b32(ms + E.N))
    edge("msg_flip", pk0, sg0, m0[:31] + bytes([m0[31] ^ 1]))

    assert list(edges) == list(EDGE_STATUS), [a for a, b in zip(edges, EDGE_STATUS) if a != b][:1]
    out_edges = []
    for name, (pk, sg, m) in edges.items():
        st = E.verify(pk, sg, m)
        assert st == EDGE_STATUS[name], (name, st)
        out_edges.append({"name": name, "pubkey": pk.hex(), "sig": sg.hex(), "msg": m.hex(), "status": st})
    counts = [sum(1 for e in out_edges if e["status"] == k) for k in range(4)]
    assert all(c >= 8 for c in counts), counts

    doc = {"comment": "generated by tests/golden/gen_ecdsa.py; statuses from tests/ecdsa_ref.py",
           "real": real, "signed": signed, "edges": out_edges}
    with open(os.path.join(HERE, "ecdsa.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("ecdsa.json: %d real, %d signed, %d edges, edge status counts %s" % (len(real), len(signed), len(out_edges),
                                                                             counts))


if __name__ == "__main__":
    main()
