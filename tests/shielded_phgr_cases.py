"""Transactions for the ZG_SHIELDED_PHGR tests (tests/test_shielded_phgr.py on the host build,
tests/test_gpu_shielded_phgr.py on the GPU), all derived from block 522's five JoinSplit transactions
(tests/golden/phgr_txs.json): a serializer for the v2 / v3 formats, the named case list, the spliced transactions and the
mixed windows. A case is (name, serialized transaction, branch id); expected values always come from
tests/shielded_phgr_ref.py.

A transaction-level index above 0 would need a proof that is valid under a key one can sign with (hSig covers the
key), which cannot be made without the proving key: desc_status is what makes the later positions observable."""
import functools

from tests import ed25519_ref
from tests import shielded_cases as C4
from tests import sighash_ref as R
from tests.conftest import load_golden

OVERWINTER_BRANCH = 0x5BA81B19
OVERWINTER_VGID = 0x03C48270
ED_SEED = C4.ED_SEED                   # the tests' own Ed25519 seed
PROOF_AT, PROOF_BYTES, DESC_BYTES = 304, 296, 1802
patch, flip = C4.patch, C4.flip

REAL = None                            # tests/golden/gen_phgr_txs.py sets it before the fixture exists


def build(t):
    """the serialized v2 / v3 transaction of a tests/sighash_ref.parse dict"""
    s = t["header"].to_bytes(4, "little")
    if t["overwintered"]:
        s += t["vgid"].to_bytes(4, "little")
    s += R.compact(len(t["inputs"]))
    for i in t["inputs"]:
        s += i["prevout"] + R.compact(len(i["script"])) + i["script"] + i["sequence"]
    s += R.compact(len(t["outputs"])) + b"".join(t["outputs"]) + t["lock_time"]
    if t["overwintered"]:
        s += t["expiry"]
    s += R.compact(len(t["joinsplits"])) + b"".join(t["joinsplits"])
    if t["joinsplits"]:
        s += t["js_pubkey"] + t["js_sig"]
    return s


def parsed(raw):
    st, t = R.parse(raw)
    assert st == R.TX_OK and t["sigver"] != 2 and t["joinsplits"]
    return dict(t)


def branch_of(t):
    return OVERWINTER_BRANCH if t["overwintered"] else 0


def sighash(t):
    return R.sighash_parsed(R.parse(build(t))[1], None, b"", 0, 1, branch_of(t))


@functools.lru_cache(maxsize=None)
def real():
    """block 522's five JoinSplit transactions; the last has two descriptions"""
    raws = REAL if REAL is not None else [bytes.fromhex(t["raw"]) for t in load_golden("phgr_txs.json")["txs"]]
    assert [len(parsed(r)["joinsplits"]) for r in raws] == [1, 1, 1, 1, 2]
    assert all(build(parsed(r)) == r for r in raws)
    return tuple(raws)


def two():
    return parsed(real()[4])


def with_proof(t, j, proof):
    return dict(t, joinsplits=t["joinsplits"][:j] + [patch(t["joinsplits"][j], PROOF_AT, proof)] + t["joinsplits"][j + 1:])


def proof_of(t, j):
    return t["joinsplits"][j][PROOF_AT:PROOF_AT + PROOF_BYTES]


def bad_proof(proof):
    """the other sign of a: still decodes, no longer verifies"""
    return flip(proof, 0)


@functools.lru_cache(maxsize=None)
def encoding_mutants():
    """the elements the prefix and x >= p mutants of pghr13.json changed: (name, offset in the proof, bytes)"""
    at = {"mut_a_prime_prefix": (33, 66), "mut_b_prefix": (66, 131), "mut_c_x_ge_p": (164, 197), "mut_b_c1_ge_p": (66, 131)}
    cs = {c["name"]: c for c in load_golden("pghr13.json")["cases"]}
    out = []
    for name, (a, b) in at.items():
        assert cs[name]["status"] == 1
        out.append((name, a, bytes.fromhex(cs[name]["proof"])[a:b]))
    return out


def own_key(t):
    """the JoinSplits under the tests' own Ed25519 key: the signature holds, hSig changes"""
    t = dict(t, js_pubkey=ed25519_ref.public_key(ED_SEED))
    return dict(t, js_sig=ed25519_ref.sign(ED_SEED, sighash(t)))


def overwinter(t):
    """the v3 transaction of the same parts: header 03000080, the Overwinter version group, an expiry height"""
    return dict(t, overwintered=True, version=3, header=0x80000003, vgid=OVERWINTER_VGID, sigver=1,
                expiry=(600).to_bytes(4, "little"))


@functools.lru_cache(maxsize=None)
def cases():
    t2 = two()
    t0 = parsed(real()[0])
    out = [("real%d" % i, r) for i, r in enumerate(real())]
    out.append(("proof_byte_1", build(with_proof(t2, 1, bad_proof(proof_of(t2, 1))))))
    for name, at, b in encoding_mutants():
        out.append(("encoding_1_" + name, build(with_proof(t2, 1, patch(proof_of(t2, 1), at, b)))))
    out.append(("own_key", build(own_key(t2))))
    out.append(("own_key_proof_byte_1", build(own_key(with_proof(t2, 1, bad_proof(proof_of(t2, 1)))))))
    for name, at, b in encoding_mutants()[:2]:
        out.append(("own_key_encoding_0_" + name, build(own_key(with_proof(t2, 0, patch(proof_of(t2, 0), at, b))))))
    out += [("ed_pubkey_invalid", build(dict(t0, js_pubkey=C4._bad_pubkey()))),
            ("ed_sig_s_high", build(dict(t0, js_sig=patch(t0["js_sig"], 63, b"\xff")))),
            ("ed_sig_bit", build(dict(t0, js_sig=flip(t0["js_sig"], 3)))),
            ("v3_same_signature", build(overwinter(t2))),
            ("v3_own_key", build(own_key(overwinter(t2))))]
    return [(n, raw, branch_of(R.parse(raw)[1])) for n, raw in out]


@functools.lru_cache(maxsize=None)
def spliced(k, j):
    """k copies of one real description under its real key (hSig does not depend on the position: the others stay
    valid), the one at j with the bad proof. The signature no longer holds: desc_status shows the positions"""
    t = parsed(real()[0])
    d = t["joinsplits"][0]
    bad = patch(d, PROOF_AT, bad_proof(d[PROOF_AT:PROOF_AT + PROOF_BYTES]))
    return build(dict(t, joinsplits=[bad if i == j else d for i in range(k)]))


def phgr_window(n_desc, fail_ends=True):
    """real transactions repeated to n_desc PHGR descriptions; the first and the last description failing (their
    transactions re-keyed, so that the transaction status shows it too)"""
    r = real()
    first = build(own_key(parsed(r[0]))) if fail_ends else r[0]
    if n_desc == 1:
        return [first]
    last = build(own_key(parsed(r[1]))) if fail_ends else r[1]
    txs, n = [first], 2
    while n < n_desc:
        k = len(txs) % 5
        d = 2 if k == 4 else 1
        if n + d > n_desc:
            k, d = 2, 1
        txs.append(r[k])
        n += d
    return txs + [last]


def mixed_window(n_phgr, n_groth=65):
    """n_phgr PHGR descriptions beside n_groth Groth16 descriptions, interleaved transaction by transaction"""
    v4, _ = C4.window(n_groth)
    pg = phgr_window(n_phgr)
    txs = []
    for i in range(max(len(v4), len(pg))):
        txs += ([v4[i]] if i < len(v4) else []) + ([pg[i]] if i < len(pg) else [])
    return txs, [branch(x) for x in txs]


def branch(raw):
    st, t = R.parse(raw)
    if t is None or t["sigver"] == 2:
        return C4.SAPLING_BRANCH
    return branch_of(t)


def interleaved_cases():
    """the f17 cases of tests/shielded_cases.py interleaved with the PHGR cases"""
    a, b = C4.cases(), cases()
    out = []
    for i in range(max(len(a), len(b))):
        out += ([a[i]] if i < len(a) else []) + ([b[i]] if i < len(b) else [])
    return out


def collector_tx(raw, **kw):
    """the zebra_amd.collector.Tx of a transaction before v4, its fields sliced out on the host as the four-call path
    takes them (zg_sighash, zg_prep_batch, zg_pghr13_verify, zg_ed25519_verify)"""
    from zebra_amd import collector as K
    t = parsed(raw)
    js = [K.JoinSplit(anchor=d[16:48], random_seed=d[208:240], nullifiers=[d[48:80], d[80:112]],
                      macs=[d[240:272], d[272:304]], commitments=[d[112:144], d[144:176]],
                      vpub_old=int.from_bytes(d[0:8], "little"), vpub_new=int.from_bytes(d[8:16], "little"),
                      zkproof=d[PROOF_AT:PROOF_AT + PROOF_BYTES], groth=False) for d in t["joinsplits"]]
    return K.Tx(js_pubkey=t["js_pubkey"], js_sig=t["js_sig"], joinsplits=js, raw=raw, branch_id=branch_of(t), **kw)


def every_tx():
    """every distinct transaction the tests above and the windows use (the fixture generator records the oracle's
    verdict for each of their (proof, inputs) pairs)"""
    txs = [c[1] for c in cases()] + [spliced(130, j) for j in (0, 63, 64, 129)]
    for n in (1, 63, 64, 65, 130):
        txs += phgr_window(n)
    return txs
