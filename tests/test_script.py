"""CPU tier of zg_inputs_verify: the oracle tests/script_ref.py pinned on the reference's
own vectors (tests/golden/inputs.json); the template matcher (zg_script_class, the library's and the host build's)
and the per-input routine the kernel runs, compiled for the CPU, against the oracle on every fixture; the matcher
again as a stand-alone program under the address and undefined-behaviour sanitizers; the kernel's resources."""
import collections
import ctypes
import shutil
import subprocess
import tempfile

import pytest

from tests import script_cases as C
from tests import script_ref as R
from tests import sighash_ref as S
from tests.conftest import load_golden
from zebra_amd import zg

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")

# kernel -> (VGPR ceiling, scratch bytes per lane, LDS bytes): the figures of profiles/f15_script_resource_usage.txt
CEILINGS = {"k_script_items": (110, 0, 0)}


def pairs(flags=0):
    """every (script_sig, script_pubkey) pair of the case list whose transaction parses"""
    txs, _, items, names, _ = C.case(flags)
    out = []
    for (t, i, pk, _), name in zip(items, names):
        st, tx = S.parse(txs[t])
        if st == S.TX_OK and i < len(tx["inputs"]):
            out.append((name, bytes(tx["inputs"][i]["script"]), bytes(pk)))
    return out


def test_oracle_hashes_are_the_references():
    g = load_golden("inputs.json")
    assert [v["fn"] for v in g["hashes"]] == ["ripemd160", "dhash160", "dhash160"]
    for v in g["hashes"]:
        assert getattr(R, v["fn"])(bytes.fromhex(v["data"])).hex() == v["hash"]
    assert R.ripemd160(b"").hex() == "9c1185a5c5e9fc54612808977ee8f548b2258d31"
    assert R.ripemd160(b"a" * 119).hex() == R.ripemd160(bytearray(b"a" * 119)).hex() != R.ripemd160(b"a" * 120).hex()


def test_oracle_verdicts_on_the_references_transactions():
    txs, br, items, flags, want, names = C.reference_vectors()
    assert len(names) == 8 and collections.Counter(want) == {R.INPUT_OK: 5, R.INPUT_HOST: 2, R.INPUT_SIGNATURE_DER: 1}
    for (t, i, pk, amount), f, w, name in zip(items, flags, want, names):
        st, _, _ = R.verify_input(txs[t], br[t], i, pk, amount, f)
        assert st == w, name
        cls, _, _, ko, kl = R.classify(S.parse(txs[t])[1]["inputs"][i]["script"], pk)
        if cls == R.SCRIPT_P2PKH:
            assert R.dhash160(S.parse(txs[t])[1]["inputs"][i]["script"][ko:ko + kl]) == pk[3:23], name
    # the Sapling-era spends verify only with their amount
    for k in (6, 7):
        t, i, pk, amount = items[k]
        assert R.verify_input(txs[t], br[t], i, pk, amount + 1, R.DERSIG)[:2] == (R.INPUT_EVAL_FALSE, 3)


def test_case_list_covers_every_status_and_detail():
    status, detail = collections.Counter(), collections.Counter()
    for flags in (0, R.DERSIG):
        _, _, _, names, (_, st, dt, _) = C.case(flags)
        status.update(st)
        detail.update(dt)
        by = dict(zip(names, zip(st, dt)))
        for n in C.PREIMAGE_LENGTHS:
            assert by["preimage/%d" % n] == ((R.INPUT_OK, 0) if n in (33, 65) else (R.INPUT_EVAL_FALSE, 1)), n
        assert all(by[k][0] == R.INPUT_HOST for k in by if k.startswith("host/"))
        assert all(by[k][0] == R.INPUT_OK for k in by if k.startswith(("pushdata/", "p2pkh/", "p2pk/")))
        assert all(by[k][0] == (R.INPUT_SIGNATURE_DER if flags else R.INPUT_EVAL_FALSE) or k == "der/valid"
                   for k in by if k.startswith("der/")), [(k, by[k]) for k in by if k.startswith("der/")]
        assert by["wrong_amount/overwinter"] == by["wrong_amount/sapling"] == (R.INPUT_EVAL_FALSE, 3)
        assert by["wrong_amount/v2"] == by["wrong_amount/v1"] == (R.INPUT_OK, 0)
    assert all(status[s] >= 4 for s in range(8)), status
    assert all(detail[d] >= 4 for d in (1, 2, 3)), detail


def test_matcher_matches_the_oracle_on_every_fixture_and_every_truncation():
    from tests import script_hostlib as H
    seen = collections.Counter()
    for name, sig, pk in pairs():
        want = R.classify(sig, pk)
        assert zg.script_class(sig, pk) == want == H.script_class(sig, pk), name
        seen[want[0]] += 1
        for k in range(len(sig)):
            assert zg.script_class(sig[:k], pk) == R.classify(sig[:k], pk), (name, k)
        for k in range(len(pk)):
            assert zg.script_class(sig, pk[:k]) == R.classify(sig, pk[:k]), (name, k)
    assert min(seen[c] for c in (0, 1, 2)) >= 9
    assert zg.script_class(b"", b"") == (0, 0, 0, 0, 0)
    L = zg.lib()
    out = (ctypes.c_uint64 * 5)()
    assert L.zg_script_class(None, 0, None, 0, out) == 0
    assert L.zg_script_class(None, 1, b"\xac", 1, out) == L.zg_script_class(b"\x00", 1, None, 1, out) == -1
    assert L.zg_script_class(b"\x00", 1, b"\xac", 1, None) == -1


def test_encoding_check_matches_the_oracle():
    from tests import script_hostlib as H
    n = 0
    for name, sig, pk in pairs():
        cls, so, sl, _, _ = R.classify(sig, pk)
        if cls:
            push = sig[so:so + sl]
            assert H.signature_encoding(push) == R.is_valid_signature_encoding(push), name
            n += 1
            for k in range(len(push)):
                assert H.signature_encoding(push[:k]) == R.is_valid_signature_encoding(push[:k]), (name, k)
    assert n > 80


@pytest.mark.parametrize("flags", [0, R.DERSIG])
def test_host_build_matches_the_oracle(flags):
    from tests import script_hostlib as H
    txs, br, items, _, want = C.case(flags)
    got = H.inputs_verify(txs, br, items, flags, threads=8)
    assert got[0] == want[0] and got[1] == want[1] and got[2] == want[2] and got[3] == want[3]


def test_standalone_matcher_under_sanitizers(tmp_path):
    """the matcher and the encoding check over heap blocks of exactly the scripts' sizes: every fixture pair and
    every proper prefix of its script_sig"""
    from tests import script_hostlib as H
    exe = H.build_program(str(tmp_path / "zg_hosttest_script"))
    lines = []
    for name, sig, pk in pairs():
        c = R.classify(sig, pk)
        enc = int(bool(c[0]) and R.is_valid_signature_encoding(sig[c[1]:c[1] + c[2]]))
        lines.append("%s %s %d %d %d %d %d %d" % ((sig.hex() or "-", pk.hex() or "-") + c + (enc,)))
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    last = r.stdout.strip().splitlines()[-1].split()
    assert last[0] == "cases" and int(last[1]) == len(lines) and int(last[3]) == 0
    assert int(last[5]) > 5000


def test_script_kernel_stays_in_registers():
    from tools import resource_table
    with tempfile.TemporaryDirectory() as tmp:
        rows = {r["name"]: r for r in resource_table.unit("zg_script.hip", tmp) if "occ" in r}
    assert len(rows) == len(CEILINGS), sorted(rows)
    for part, (vgpr, scratch, lds) in CEILINGS.items():
        (name, r), = [(n, r) for n, r in rows.items() if part in n]
        assert r["vgpr"] <= vgpr and r["scratch"] <= scratch and r["lds"] <= lds, (name, r)
        assert r.get("vspill", 0) == 0 and r.get("sspill", 0) == 0 and r["occ"] >= 2, (name, r)


def test_abi_exports_and_constants():
    L = zg.lib()
    assert hasattr(L, "zg_inputs_verify") and hasattr(L, "zg_script_class")
    hdr = open(zg.HERE + "/../include/zg.h").read()
    for name, v in (("SCRIPT_HOST", 0), ("SCRIPT_P2PKH", 1), ("SCRIPT_P2PK", 2), ("SCRIPT_VERIFY_DERSIG", 1),
                    ("INPUT_OK", 0), ("INPUT_EQUALVERIFY", 1), ("INPUT_SIGNATURE_DER", 2), ("INPUT_EVAL_FALSE", 3),
                    ("INPUT_HOST", 4), ("INPUT_TX_MALFORMED", 5), ("INPUT_TX_NONCANONICAL", 6), ("INPUT_RANGE", 7)):
        assert "#define ZG_%s %d" % (name, v) in hdr and getattr(zg, name) == v == getattr(R, name.replace("SCRIPT_VERIFY_", ""), v)


# ------------------------------------------------------------------ the collector, with a stand-in verifier
def oracle_backend(calls):
    def inputs_verify(txs, branch_ids, items, flags):
        calls.append((len(txs), len(items), flags))
        return R.run(txs, branch_ids, items, flags)
    return inputs_verify


def template_window(flags=R.DERSIG):
    from zebra_amd.collector import Prevout, Tx
    tt = C.template_txs(flags)
    return [Tx(raw=raw, branch_id=b, sighash=bytes(32), prevouts=[Prevout(pk, a) for pk, a in outs]) for raw, b, outs, _ in tt], \
        [e for _, _, _, e in tt]


def test_collector_places_the_template_error_where_the_eval_error_stands():
    from zebra_amd.collector import Tx, verify_block
    txs, errors = template_window()
    assert len(txs) > 60 and {e[2] for e in errors if e} == {"EqualVerify", "SignatureDer", "EvalFalse"}
    assert any(e and e[1] == 1 for e in errors)                  # a failing input that is not the first
    good = [t for t, e in zip(txs, errors) if e is None]
    calls = []
    kw = dict(verify=lambda *a: [], inputs_verify=oracle_backend(calls))
    assert verify_block(good, **kw) is None and calls == [(len(good), sum(len(t.prevouts) for t in good), R.DERSIG)]
    first = next(k for k, e in enumerate(errors) if e)
    assert verify_block(txs, **kw) == (first, errors[first])     # the lowest failing transaction, its lowest input
    for k, e in enumerate(errors):
        if e:
            w = good[:2] + [txs[k]] + good[2:4]
            assert verify_block(w, **kw) == (2, e)
    # the flags are the window's argument: the reference's 124276 transaction fails only under DERSIG
    off, off_errors = template_window(0)
    calls.clear()
    first0 = next(k for k, e in enumerate(off_errors) if e)
    assert verify_block(off, script_flags=0, **kw) == (first0, off_errors[first0]) and calls[-1][2] == 0
    assert "SignatureDer" not in {e[2] for e in off_errors if e} and off_errors.count(None) > errors.count(None)
    # after pre_error, before the JoinSplit stage
    from dataclasses import replace
    bad = txs[first]
    assert verify_block([replace(bad, pre_error="Maturity")], **kw) == (0, "Maturity")
    from zebra_amd.collector import JoinSplit
    js = dict(js_pubkey=None, js_sig_ok=False, joinsplits=[JoinSplit(bytes(32), bytes(32), [bytes(32)] * 2, [bytes(32)] * 2,
                                                                     [bytes(32)] * 2, 0, 0, bytes(192), pghr_ok=True)])
    assert verify_block([replace(bad, **js)], **kw) == (0, errors[first])
    assert verify_block([replace(good[0], **js)], **kw) == (0, "JoinSplitSignature")
    # transactions without prevouts take the other paths in the same window, untouched
    calls.clear()
    assert verify_block([Tx(), good[0], Tx(pre_error="Input")], **kw) == (2, "Input") and calls[0][:2] == (1, len(good[0].prevouts))
    assert verify_block([Tx(), Tx()], **kw) is None and len(calls) == 1     # no prevouts: no call


def test_collector_rejects_mixed_fields_and_items_without_a_verdict():
    from dataclasses import replace
    from zebra_amd.collector import EcdsaCheck, EcdsaRequest, verify_block
    txs, errors = template_window()
    good = next(t for t, e in zip(txs, errors) if e is None)
    kw = dict(verify=lambda *a: [], inputs_verify=oracle_backend([]))
    for broken in (replace(good, raw=None), replace(good, branch_id=None),
                   replace(good, ecdsa_checks=[EcdsaCheck(0, b"", b"", bytes(32))]),
                   replace(good, ecdsa_requests=[EcdsaRequest(0, b"", b"", b"", 1, 0)]),
                   replace(good, eval_rerun=lambda lookup: None)):
        with pytest.raises(ValueError):
            verify_block([broken], **kw)
    with pytest.raises(zg.ZgError):                      # no backend
        verify_block([good], verify=lambda *a: [])
    from zebra_amd.collector import Prevout
    for broken in (replace(good, prevouts=[Prevout(b"\x51", 0)] + good.prevouts[1:]),       # HOST
                   replace(good, prevouts=good.prevouts + [good.prevouts[0]]),              # RANGE
                   replace(good, raw=good.raw[:-1])):                                       # TX_MALFORMED
        with pytest.raises(zg.ZgError):
            verify_block([broken], **kw)
