"""CPU tier of zg_inputs_verify's multisig classes: the oracle tests/multisig_ref.py pinned
on the reference's own 2-of-3 vector; the case list's coverage; the matcher (zg_script_match, the library's and the
host build's) and the routines the multisig kernels run, compiled for the CPU, against the oracle on every case; the
matcher again as a stand-alone program under the address and undefined-behaviour sanitizers; the kernels' resources."""
import collections
import ctypes
import shutil
import subprocess
import tempfile

import pytest

from tests import multisig_cases as C
from tests import multisig_ref as M
from tests import script_ref as R
from tests import sighash_ref as S
from zebra_amd import zg

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")

BIT = M.TEMPLATE_MULTISIG
# kernel -> (VGPR ceiling, scratch bytes per lane, LDS bytes): the figures of profiles/f16_multisig_resource_usage.txt
CEILINGS = {"k_multisig_items": (105, 0, 0), "k_multisig_rows": (42, 0, 0), "k_multisig_fold": (13, 0, 0)}


def pairs():
    """every (name, script_sig, script_pubkey) of the case list whose transaction parses"""
    txs, _, items, names, _ = C.case(BIT)
    out = []
    for (t, i, pk, _), name in zip(items, names):
        st, tx = S.parse(txs[t])
        if st == S.TX_OK and i < len(tx["inputs"]):
            out.append((name, bytes(tx["inputs"][i]["script"]), bytes(pk)))
    return out


def redeem_truncations(sig, pk):
    """a P2SH multisig script_sig with every proper prefix of its redeem script pushed in the script's place"""
    mt = M.match(sig, pk, BIT)
    if mt[0] != M.SCRIPT_P2SH_MULTISIG:
        return []
    red = sig[mt[3]:mt[3] + mt[4]]
    head = sig[:M.pushes(sig)[-1][2]]
    return [head + R.push(red[:k]) for k in range(len(red))]


def reference_vector():
    txs, br, items, _, want, names = C.reference_vectors()
    k = names.index("test_check_transaction_multisig")
    assert want[k] == R.INPUT_HOST
    t, i, pk, amount = items[k]
    return txs[t], br[t], i, pk, amount


def test_oracle_on_the_references_multisig_vector():
    raw, branch, i, pk, amount = reference_vector()
    sig = bytes(S.parse(raw)[1]["inputs"][i]["script"])
    mt = M.match(sig, pk, BIT)
    assert mt[:3] == (M.SCRIPT_P2SH_MULTISIG, 2, 3) and mt[4:6] == (201, 4) and mt[3] + mt[4] == len(sig)
    code = sig[mt[3]:]
    assert R.dhash160(code) == pk[2:22]
    for flags in (0, R.DERSIG):
        assert M.verify_input(raw, branch, i, pk, amount, flags) == (R.INPUT_HOST, 0, R.ZERO)
        assert M.match(sig, pk, flags) == (0,) * 8
    for flags in (BIT, BIT | R.DERSIG):
        st, dt, h = M.verify_input(raw, branch, i, pk, amount, flags)
        assert (st, dt) == (R.INPUT_OK, 0)
        # the walk, in the reference's numbering (push order): (signature 1, key 2) passes, (0, 1) fails with
        # ECDSA_SIGNATURE, (0, 0) passes; the hash reported is that of the last pair, signature 0's
        m, n, key_at = M.multisig_form(code)
        keys = [code[o:o + l] for o, l in key_at]
        sigs = [sig[o:o + l] for o, l, _ in M.pushes(sig)[1:3]]
        hs = [S.sighash_parsed(S.parse(raw)[1], i, code, amount, s[-1], branch) for s in sigs]
        from tests import ecdsa_ref as E
        assert [E.verify(keys[k], sigs[s][:-1], hs[s]) for s, k in ((1, 2), (0, 1), (0, 0))] == [0, 3, 0]
        assert h == hs[0] != R.ZERO


def test_case_list_covers_every_verdict():
    seen = collections.Counter()
    for flags in (BIT, BIT | R.DERSIG):
        _, _, _, names, (_, st, dt, hs) = C.case(flags)
        seen.update(zip(st, dt))
        by = dict(zip(names, zip(st, dt, hs)))
        assert all(by[k][0] == R.INPUT_HOST for k in by if k.startswith("host/")), [k for k in by if k.startswith("host/") and by[k][0] != 4]
        assert all(by[k][:2] == (R.INPUT_OK, 0) and by[k][2] != R.ZERO for k in by
                   if k.startswith(("mn/", "wide/", "2of5/", "hashtypes/", "dummy/", "redeem_push/", "padding/")))
        assert all(by[k][:2] == (R.INPUT_SIGNATURE_DER, 0) if flags & R.DERSIG else by[k][0] in (R.INPUT_OK, R.INPUT_EVAL_FALSE)
                   for k in by if k.startswith("der/reached"))
        assert by["der/never_reached"][:2] == by["empty/unreached"][:2] == (R.INPUT_EVAL_FALSE, 3)
        assert all(by[k] == (R.INPUT_EVAL_FALSE, 0, R.ZERO) for k in by if k.startswith("mismatch/"))
        assert by["empty/only"] == (R.INPUT_EVAL_FALSE, 2, R.ZERO) and by["key05/fails"][:2] == (R.INPUT_EVAL_FALSE, 1)
        assert [by["2of3/%d%d" % (a, c)][0] for a in range(3) for c in range(3)] == [3, 0, 0, 3, 3, 0, 3, 3, 3]
        assert by["mixed/bare_fails"][:2] == (R.INPUT_EVAL_FALSE, 3) and by["mixed/p2sh"][0] == by["mixed/p2pk"][0] == 0
        assert by["test_check_transaction_multisig"][:2] == (R.INPUT_OK, 0)
    for want in ((R.INPUT_OK, 0), (R.INPUT_SIGNATURE_DER, 0), (R.INPUT_HOST, 0), (R.INPUT_EVAL_FALSE, 0),
                 (R.INPUT_EVAL_FALSE, 1), (R.INPUT_EVAL_FALSE, 2), (R.INPUT_EVAL_FALSE, 3)):
        assert seen[want] >= 2, (want, seen)
    # without the bit the oracle is script_ref: every multisig item HOST
    for flags in (0, R.DERSIG):
        txs, br, items, _, want = C.case(flags)
        assert want == R.run(txs, br, items, flags) and collections.Counter(want[1])[R.INPUT_HOST] > 130


def test_matcher_matches_the_oracle_on_every_case_and_every_truncation():
    from tests import multisig_hostlib as H
    seen = collections.Counter()
    for name, sig, pk in pairs():
        want = M.match(sig, pk, BIT)
        assert zg.script_match(sig, pk, BIT) == want == H.script_match(sig, pk, BIT), name
        assert zg.script_match(sig, pk, BIT | R.DERSIG) == want
        seen[want[0]] += 1
        for flags in (0, R.DERSIG):                                   # without the bit: zg_script_class's class
            assert zg.script_match(sig, pk, flags)[0] == zg.script_class(sig, pk)[0] == M.match(sig, pk, flags)[0], name
        for k in range(len(sig)):
            assert zg.script_match(sig[:k], pk, BIT) == M.match(sig[:k], pk, BIT), (name, k)
        if want[0] == M.SCRIPT_MULTISIG:
            for k in range(len(pk)):
                assert zg.script_match(sig, pk[:k], BIT) == M.match(sig, pk[:k], BIT), (name, k)
        for cut in redeem_truncations(sig, pk):
            assert zg.script_match(cut, pk, BIT) == M.match(cut, pk, BIT) and M.match(cut, pk, BIT)[0] == 0, (name, len(cut))
    assert min(seen[c] for c in range(5)) >= 3 and seen[3] >= 40 and seen[4] >= 40, seen
    assert zg.script_match(b"", b"", BIT) == (0,) * 8
    L = zg.lib()
    out = (ctypes.c_uint64 * 8)()
    assert L.zg_script_match(None, 0, None, 0, BIT, out) == 0
    assert L.zg_script_match(None, 1, b"\xac", 1, BIT, out) == L.zg_script_match(b"\x00", 1, None, 1, BIT, out) == -1
    assert L.zg_script_match(b"\x00", 1, b"\xac", 1, BIT, None) == -1
    assert L.zg_script_match(b"\x00", 1, b"\xac", 1, 2, out) == L.zg_script_match(b"\x00", 1, b"\xac", 1, BIT | 4, out) == -1


@pytest.mark.parametrize("flags", [BIT, BIT | R.DERSIG])
def test_host_build_matches_the_oracle(flags):
    from tests import multisig_hostlib as H
    txs, br, items, _, want = C.case(flags)
    got = H.inputs_verify(txs, br, items, flags, threads=8)
    assert got[0] == want[0] and got[1] == want[1] and got[2] == want[2] and got[3] == want[3]


def test_standalone_matcher_under_sanitizers(tmp_path):
    """the matcher over heap blocks of exactly the scripts' sizes: every case, every proper prefix of its script_sig
    and of its script_pubkey, and every proper prefix of its redeem script pushed in the script's place"""
    from tests import multisig_hostlib as H
    exe = H.build_program(str(tmp_path / "zg_hosttest_multisig"))
    lines = []
    for name, sig, pk in pairs():
        for s in [sig] + redeem_truncations(sig, pk)[::7]:
            lines.append("%s %s %d %d %d %d %d %d %d %d %d" % ((s.hex() or "-", pk.hex() or "-", BIT) + M.match(s, pk, BIT)))
        lines.append("%s %s %d %d %d %d %d %d %d %d %d" % ((sig.hex() or "-", pk.hex() or "-", 0) + M.match(sig, pk, 0)))
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    last = r.stdout.strip().splitlines()[-1].split()
    assert last[0] == "cases" and int(last[1]) == len(lines) and int(last[3]) == 0
    assert int(last[5]) > 20000


def test_multisig_kernels_stay_in_registers():
    from tools import resource_table
    with tempfile.TemporaryDirectory() as tmp:
        rows = {r["name"]: r for r in resource_table.unit("zg_multisig.hip", tmp) if "occ" in r}
    assert len(rows) == len(CEILINGS), sorted(rows)
    for part, (vgpr, scratch, lds) in CEILINGS.items():
        (name, r), = [(n, r) for n, r in rows.items() if part in n]
        assert r["vgpr"] <= vgpr and r["scratch"] <= scratch and r["lds"] <= lds, (name, r)
        assert r.get("vspill", 0) == 0 and r.get("sspill", 0) == 0 and r["occ"] >= 4, (name, r)


def test_abi_exports_and_constants():
    L = zg.lib()
    assert hasattr(L, "zg_script_match")
    hdr = open(zg.HERE + "/../include/zg.h").read()
    for name, v in (("SCRIPT_MULTISIG", 3), ("SCRIPT_P2SH_MULTISIG", 4), ("SCRIPT_TEMPLATE_MULTISIG", 0x100)):
        assert "#define ZG_%s %d" % (name, v) in hdr and getattr(zg, name) == v
    assert (M.SCRIPT_MULTISIG, M.SCRIPT_P2SH_MULTISIG, M.TEMPLATE_MULTISIG) == (3, 4, 0x100)


# ------------------------------------------------------------------ the collector, with a stand-in verifier
def window(flags, corrupt=None):
    """one all-multisig transaction, one mixing a P2PKH, a P2PK and two multisig inputs, and a P2PKH-only one"""
    from zebra_amd.collector import Prevout, Tx
    tt = C.verdict_txs(flags)
    pick = [next(v for v in tt if v[3] is None and set(v[4]) == {3, 4}),
            next(v for v in tt if v[3] is None and {1, 2, 3, 4} & set(v[4]) == {2, 3, 4}),
            next(v for v in tt if v[3] is None and set(v[4]) == {1})]
    return [Tx(raw=raw, branch_id=b, sighash=bytes(32), prevouts=[Prevout(pk, a) for pk, a in outs]) for raw, b, outs, _, _ in pick]


def test_collector_hands_the_windows_flags_to_the_verifier():
    from zebra_amd.collector import verify_block
    calls = []

    def backend(txs, branch_ids, items, flags):
        calls.append((len(txs), len(items), flags))
        return M.run(txs, branch_ids, items, flags)
    kw = dict(verify=lambda *a: [], inputs_verify=backend)
    w = window(BIT | R.DERSIG)
    assert verify_block(w, script_flags=BIT | R.DERSIG, **kw) is None
    assert calls == [(3, sum(len(t.prevouts) for t in w), BIT | R.DERSIG)]
    with pytest.raises(zg.ZgError):                                  # without the bit a multisig input has no verdict
        verify_block(w, **kw)
    failing = next(v for v in C.verdict_txs(BIT | R.DERSIG) if v[3] and 3 in v[4] and v[3][1] > 0)
    from zebra_amd.collector import Prevout, Tx
    bad = Tx(raw=failing[0], branch_id=failing[1], sighash=bytes(32), prevouts=[Prevout(pk, a) for pk, a in failing[2]])
    assert verify_block(w[:2] + [bad] + w[2:], script_flags=BIT | R.DERSIG, **kw) == (2, failing[3])
