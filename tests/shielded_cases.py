"""Transactions for the zg_shielded_verify tests (tests/test_shielded.py on the host build, tests/test_gpu_shielded.py
on the GPU), all derived from the whole, valid transactions of tests/golden: a serializer for the v4 format, the
named case list and the spliced windows. A case is (name, serialized transaction, branch id); expected values always
come from tests/shielded_ref.py."""
import functools

from oracle import sapling_sig
from tests import ed25519_ref
from tests import sighash_ref as R
from tests.conftest import load_golden

SAPLING_BRANCH = 0x76B809BB
SPEND_SK = 0x1234567890ABCDEF1234567890ABCDEF       # the tests' own RedJubjub key
ED_SEED = bytes(range(32))                           # ... and Ed25519 seed
I64_MIN = (-(1 << 63)).to_bytes(8, "little", signed=True)


def build(t, count=R.compact):
    """the serialized v4 transaction of a tests/sighash_ref.parse dict; count: the encoder of the spend count"""
    s = t["header"].to_bytes(4, "little") + t["vgid"].to_bytes(4, "little") + R.compact(len(t["inputs"]))
    for i in t["inputs"]:
        s += i["prevout"] + R.compact(len(i["script"])) + i["script"] + i["sequence"]
    s += R.compact(len(t["outputs"])) + b"".join(t["outputs"]) + t["lock_time"] + t["expiry"] + t["value_balance"]
    s += count(len(t["spends"])) + b"".join(t["spends"]) + R.compact(len(t["soutputs"])) + b"".join(t["soutputs"])
    s += R.compact(len(t["joinsplits"])) + b"".join(t["joinsplits"])
    if t["joinsplits"]:
        s += t["js_pubkey"] + t["js_sig"]
    if t["spends"] or t["soutputs"]:
        s += t["binding_sig"]
    return s


def parsed(raw):
    st, t = R.parse(raw)
    assert st == R.TX_OK and t["sigver"] == 2
    return dict(t)


def patch(b, at, new):
    return b[:at] + bytes(new) + b[at + len(new):]


def flip(b, at, bit=1):
    return patch(b, at, [b[at] ^ bit])


def sighash(t):
    return R.sighash_parsed(R.parse(build(t))[1], None, b"", 0, 1, SAPLING_BRANCH)


@functools.lru_cache(maxsize=None)
def real():
    """the six whole transactions: sap0 and sap2 (one spend, one output), sap1 (a transparent input, one output), js0..2
    (one Groth JoinSplit each), and the v4 transaction with transparent inputs only"""
    g = load_golden("sighash.json")
    out = {"sap%d" % i: bytes.fromhex(v["tx"]) for i, v in enumerate(g["sapling"])}
    out.update({"js%d" % i: bytes.fromhex(v["tx"]) for i, v in enumerate(g["joinsplit"])})
    out["transparent"] = bytes.fromhex(g["sapling_spends"][1]["tx"])
    assert [len(parsed(out[k])["spends"]) for k in ("sap0", "sap1", "sap2")] == [1, 0, 1]
    t = parsed(out["transparent"])
    assert not (t["spends"] or t["soutputs"] or t["joinsplits"]) and t["value_balance"] == bytes(8)
    return out


SIX = ("sap0", "sap1", "sap2", "js0", "js1", "js2")


def own_spend(t, j, proof=None):
    """spend j under the tests' own key: rk and, over the new hash, spend_auth_sig; proof: replaces the proof"""
    s = patch(t["spends"][j], 96, sapling_sig.public_key(SPEND_SK, sapling_sig.GEN_SPEND_AUTH))
    if proof is not None:
        s = patch(s, 128, proof)
    t = dict(t, spends=t["spends"][:j] + [s] + t["spends"][j + 1:])
    sig = sapling_sig.redjubjub_sign(SPEND_SK, s[96:128] + sighash(t), sapling_sig.GEN_SPEND_AUTH, bytes(80))
    return dict(t, spends=t["spends"][:j] + [patch(s, 320, sig)] + t["spends"][j + 1:])


def own_joinsplit_key(t):
    """the JoinSplits under the tests' own Ed25519 key: the signature holds, hSig changes"""
    t = dict(t, js_pubkey=ed25519_ref.public_key(ED_SEED))
    return dict(t, js_sig=ed25519_ref.sign(ED_SEED, sighash(t)))


def _bad_pubkey():
    for i in range(256):
        b = bytes([i]) + bytes(31)
        if ed25519_ref.decompress(b) is None:
            return b
    raise AssertionError


@functools.lru_cache(maxsize=None)
def cases():
    r = real()
    prep = load_golden("input_prep.json")["prep_errors"]
    legacy = bytes.fromhex(load_golden("sighash.json")["legacy"][0]["tx"])
    v3 = [bytes.fromhex(v["tx"]) for v in load_golden("sapling_sigs.json")["sighash_vectors"]]
    v3 = {bool(R.parse(x)[1]["joinsplits"]): x for x in v3 if R.parse(x)[1]["sigver"] == 1}
    out = [(k, r[k]) for k in SIX]
    tr = parsed(r["transparent"])
    out += [("transparent", r["transparent"]), ("transparent_vb1", build(dict(tr, value_balance=(1).to_bytes(8, "little")))),
            ("transparent_vb_min", build(dict(tr, value_balance=I64_MIN))),
            ("v1", legacy), ("v3_none", v3[False]), ("v3_host", v3[True]), ("truncated", r["sap0"][:-1]),
            ("noncanonical", build(parsed(r["sap0"]), count=lambda n: b"\xfd" + n.to_bytes(2, "little")))]
    sap0, sap1 = parsed(r["sap0"]), parsed(r["sap1"])
    at = {"cv": 0, "anchor": 32, "rk": 96, "cmu": 32, "epk": 64}
    for e in prep:
        f = e["name"].split("_")[0]
        if e["kind"] == "spend":
            t = dict(sap0, spends=[patch(sap0["spends"][0], at[f], bytes.fromhex(e["fields"][f]))])
        else:
            t = dict(sap1, soutputs=[patch(sap1["soutputs"][0], at[f], bytes.fromhex(e["fields"][f]))])
        out.append(("%s_%s" % (e["kind"], e["name"]), build(t)))
    out += [("spend_auth_sig_bit", build(dict(sap0, spends=[flip(sap0["spends"][0], 320 + 40)]))),
            ("binding_sig_bit", build(dict(sap0, binding_sig=flip(sap0["binding_sig"], 5)))),
            ("balance_min", build(dict(sap1, value_balance=I64_MIN))),
            ("ciphertext_byte", build(dict(sap1, soutputs=[flip(sap1["soutputs"][0], 200)]))),
            ("ciphertext_byte_spend", build(dict(sap0, soutputs=[flip(sap0["soutputs"][0], 200)]))),
            ("spend_proof_byte", build(dict(sap0, spends=[flip(sap0["spends"][0], 128 + 50)]))),
            ("spend_own_key", build(own_spend(sap0, 0))),
            ("spend_own_key_bad_proof", build(own_spend(sap0, 0, b"\xff" * 192))),
            ("output_proof_byte", build(dict(sap1, soutputs=[flip(sap1["soutputs"][0], 756 + 50)]))),
            ("output_proof_other", build(dict(sap1, soutputs=[patch(sap1["soutputs"][0], 756, sap0["soutputs"][0][756:])]))),
            ("output_proof_undecodable", build(dict(sap1, soutputs=[patch(sap1["soutputs"][0], 756, b"\xff" * 192)])))]
    js0, js1 = parsed(r["js0"]), parsed(r["js1"])
    out += [("js_sig_bit", build(dict(js0, js_sig=flip(js0["js_sig"], 3)))),
            ("js_sig_s_high", build(dict(js0, js_sig=patch(js0["js_sig"], 63, b"\xff")))),
            ("js_pubkey_invalid", build(dict(js0, js_pubkey=_bad_pubkey()))),
            ("js_own_key", build(own_joinsplit_key(js0))),
            ("js_own_key_bad_proof",
             build(own_joinsplit_key(dict(js0, joinsplits=[patch(js0["joinsplits"][0], 304, b"\xff" * 192)])))),
            ("js_proof_byte", build(dict(js0, joinsplits=[flip(js0["joinsplits"][0], 304 + 50)])))]
    for j in (0, 2):
        out += [("outputs3_bad%d" % j, spliced_outputs(3, j)), ("joinsplits3_foreign%d" % j, spliced_joinsplits(3, j)),
                ("spends3_bad%d" % j, spliced_spends(3, j))]
    out.append(("js_and_sapling", build(dict(sap0, joinsplits=js1["joinsplits"], js_pubkey=js1["js_pubkey"],
                                             js_sig=js1["js_sig"]))))
    return [(n, raw, SAPLING_BRANCH) for n, raw in out]


def _small_order_cv():
    e = [e for e in load_golden("input_prep.json")["prep_errors"] if e["name"] == "cv_small_order"][0]
    return bytes.fromhex(e["fields"]["cv"])


def spliced_outputs(k, j):
    """k verbatim copies of a valid output (an output carries no signature: each passes on its own), the one at j
    with a small-order cv"""
    t = parsed(real()["sap1"])
    o = t["soutputs"][0]
    return build(dict(t, soutputs=[patch(o, 0, _small_order_cv()) if i == j else o for i in range(k)]))


def spliced_joinsplits(k, j):
    """k copies of one JoinSplit under its original pubkey, another transaction's description at j"""
    t, other = parsed(real()["js0"]), parsed(real()["js1"])
    return build(dict(t, joinsplits=[other["joinsplits"][0] if i == j else t["joinsplits"][0] for i in range(k)]))


def spliced_spends(k, j):
    """k copies of one spend, the one at j with a small-order cv"""
    t = parsed(real()["sap0"])
    s = t["spends"][0]
    return build(dict(t, spends=[patch(s, 0, _small_order_cv()) if i == j else s for i in range(k)]))


def window(n_desc):
    """real transactions repeated to n_desc descriptions, a failing description in the first and in the last slot"""
    r = real()
    first, last = spliced_outputs(1, 0), build(dict(parsed(r["sap1"]), soutputs=[
        patch(parsed(r["sap1"])["soutputs"][0], 756, b"\xff" * 192)]))
    txs, n = [first], 2
    while n < n_desc:
        k = SIX[len(txs) % 6]
        d = 2 if k in ("sap0", "sap2") else 1
        if n + d > n_desc:
            k, d = "js0", 1
        txs.append(r[k])
        n += d
    return txs + [last], [SAPLING_BRANCH] * (len(txs) + 1)


def collector_tx(raw, branch_id=SAPLING_BRANCH, **kw):
    """the zebra_amd.collector.Tx of a v4 transaction, its fields sliced out on the host as the six-call path takes
    them"""
    from zebra_amd import collector as K
    t = parsed(raw)
    js = [K.JoinSplit(anchor=d[16:48], random_seed=d[208:240], nullifiers=[d[48:80], d[80:112]],
                      macs=[d[240:272], d[272:304]], commitments=[d[112:144], d[144:176]],
                      vpub_old=int.from_bytes(d[0:8], "little"), vpub_new=int.from_bytes(d[8:16], "little"),
                      zkproof=d[304:496]) for d in t["joinsplits"]]
    sp = [K.Spend(cv=s[0:32], anchor=s[32:64], nullifier=s[64:96], rk=s[96:128], zkproof=s[128:320],
                  spend_auth_sig=s[320:384]) for s in t["spends"]]
    out = [K.Output(cv=o[0:32], cmu=o[32:64], epk=o[64:96], zkproof=o[756:948]) for o in t["soutputs"]]
    return K.Tx(js_pubkey=t["js_pubkey"], js_sig=t.get("js_sig"), joinsplits=js, spends=sp, outputs=out,
                value_balance=int.from_bytes(t["value_balance"], "little", signed=True),
                binding_sig=t.get("binding_sig"), raw=raw, branch_id=branch_id, **kw)
