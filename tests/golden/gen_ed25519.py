#!/usr/bin/env python3
"""Generate tests/golden/ed25519.json: the fixtures of the Ed25519 JoinSplit signature check.

Reads the reference as TEXT only, the way gen_golden.py does (block 419221,
test-data/src/lib.rs:117-131): the three JoinSplit-bearing transactions' (pubkey, signature) are
taken from the raw bytes (the 64 bytes before binding_sig, or the last 64 bytes when there is
none), the message is the oracle's ZIP-243 no-input sighash. Every expected status comes from
tests/ed25519_ref.py; the generator asserts the three real signatures and RFC 8032 TEST 1 verify,
each named edge case has the status listed in EDGE_STATUS, and every status 0-3 occurs twice.

    python tests/golden/gen_ed25519.py
"""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

import ed25519_ref as E  # noqa: E402

EDGE_STATUS = {"pk_not_on_curve": 1, "pk_bad_and_s_high": 1, "s_bit253": 2, "s_bit254": 2, "s_bit255": 2,
               "s_plus_l": 0, "msg_flip": 3, "r_flip": 3, "other_valid_key": 3, "a_identity_noncanonical": 0,
               "a_x0_signbit": 0, "a_order8": 0, "r_identity_ok": 0, "r_noncanonical": 3, "r_identity_signbit": 3,
               "all_zero": None}


def real_entries():
    from gen_golden import extract_sources
    from oracle import sapling_sig as S, zcash as Z
    _, _, _, block_hex, _ = extract_sources()
    rd = Z._Reader(bytes.fromhex(block_hex))
    rd.take(140)
    rd.take(rd.compact())
    out = []
    for _ in range(rd.compact()):
        o0 = rd.o
        t = Z.parse_tx(rd)
        raw = rd.d[o0:rd.o]
        p = S.parse_tx_raw(raw)
        if not p["joinsplits"]:
            continue
        sig = E.joinsplit_sig_from_raw(raw, "binding_sig" in p)
        out.append({"txid": t["txid"], "pubkey": p["js_pubkey"].hex(), "sig": sig.hex(),
                    "sighash": S.sighash(p, None, b"", 0, 1).hex()})
    return out


def order8_point():
    """a point of order exactly 8: [l] P for the first decodable y whose [l] P has order 8"""
    y = 2
    while True:
        p = E.decompress(y.to_bytes(32, "little"))
        if p is not None:
            q = E.mul(E.L, p)
            if E.compress(E.mul(4, q)) != E.compress(E.IDENTITY):
                return q
        y += 1


def main():
    rnd = random.Random(25519)
    real = real_entries()
    assert len(real) == 3
    for e in real:
        assert E.verify(bytes.fromhex(e["pubkey"]), bytes.fromhex(e["sig"]), bytes.fromhex(e["sighash"])) == 0, e["txid"]
    t1 = E.RFC8032_TEST1
    assert E.public_key(bytes.fromhex(t1["seed"])).hex() == t1["pubkey"]
    assert E.sign(bytes.fromhex(t1["seed"]), b"").hex() == t1["sig"]
    assert E.verify(bytes.fromhex(t1["pubkey"]), bytes.fromhex(t1["sig"]), b"") == 0

    signed = []
    for i in range(48):
        seed, msg = rnd.randbytes(32), rnd.randbytes(32)
        signed.append({"seed": seed.hex(), "pubkey": E.public_key(seed).hex(), "sig": E.sign(seed, msg).hex(),
                       "msg": msg.hex()})
        assert E.verify(bytes.fromhex(signed[-1]["pubkey"]), bytes.fromhex(signed[-1]["sig"]), msg) == 0

    pk0, sg0, m0 = (bytes.fromhex(real[0][k]) for k in ("pubkey", "sig", "sighash"))
    edges = {}

    def edge(name, pk, sg, m):
        edges[name] = (bytes(pk), bytes(sg), bytes(m))

    y = 2
    while E.decompress(y.to_bytes(32, "little")) is not None:
        y += 1
    bad_pk = y.to_bytes(32, "little")
    edge("pk_not_on_curve", bad_pk, sg0, m0)
    edge("pk_bad_and_s_high", bad_pk, sg0[:63] + bytes([sg0[63] | 0x80]), m0)
    for bit in (253, 254, 255):
        s = int.from_bytes(sg0[32:], "little") | (1 << bit)
        edge("s_bit%d" % bit, pk0, sg0[:32] + s.to_bytes(32, "little"), m0)
    s = int.from_bytes(sg0[32:], "little") + E.L
    assert s < 2 ** 253
    edge("s_plus_l", pk0, sg0[:32] + s.to_bytes(32, "little"), m0)
    edge("msg_flip", pk0, sg0, bytes([m0[0] ^ 1]) + m0[1:])
    edge("r_flip", pk0, bytes([sg0[0] ^ 1]) + sg0[1:], m0)
    edge("other_valid_key", bytes.fromhex(real[1]["pubkey"]), sg0, m0)
    # A = identity: R' = [S]B whatever k is
    s = rnd.randrange(E.L)
    r = E.compress(E.mul(s, E.B))
    edge("a_identity_noncanonical", (E.P + 1).to_bytes(32, "little"), r + s.to_bytes(32, "little"), rnd.randbytes(32))
    edge("a_x0_signbit", bytes([1] + [0] * 30 + [0x80]), r + s.to_bytes(32, "little"), rnd.randbytes(32))
    # A of order 8, R = [S]B: valid iff k = 0 mod 8 (searched over S)
    a8 = E.compress(order8_point())
    m8 = rnd.randbytes(32)
    s = 1
    while True:
        r = E.compress(E.mul(s, E.B))
        k = int.from_bytes(__import__("hashlib").sha512(r + a8 + m8).digest(), "little") % E.L
        if k % 8 == 0:
            break
        s += 1
    edge("a_order8", a8, r + s.to_bytes(32, "little"), m8)
    ident = bytes([1] + [0] * 31)
    m = rnd.randbytes(32)
    edge("r_identity_ok", ident, ident + bytes(32), m)
    edge("r_noncanonical", ident, (E.P + 1).to_bytes(32, "little") + bytes(32), m)
    edge("r_identity_signbit", ident, bytes([1] + [0] * 30 + [0x80]) + bytes(32), m)
    edge("all_zero", bytes(32), bytes(64), bytes(32))

    assert list(edges) == list(EDGE_STATUS)
    out_edges = []
    for name, (pk, sg, m) in edges.items():
        st = E.verify(pk, sg, m)
        assert EDGE_STATUS[name] is None or st == EDGE_STATUS[name], (name, st)
        out_edges.append({"name": name, "pubkey": pk.hex(), "sig": sg.hex(), "msg": m.hex(), "status": st})
    counts = [sum(1 for e in out_edges if e["status"] == k) + (len(real) + len(signed) if k == 0 else 0)
              for k in range(4)]
    assert all(c >= 2 for c in counts), counts

    doc = {"comment": "generated by tests/golden/gen_ed25519.py; statuses from tests/ed25519_ref.py",
           "real": real, "rfc8032": [t1], "signed": signed, "edges": out_edges}
    with open(os.path.join(HERE, "ed25519.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("ed25519.json: %d real, %d signed, %d edges, status counts %s" % (len(real), len(signed), len(out_edges),
                                                                            counts))


if __name__ == "__main__":
    main()
