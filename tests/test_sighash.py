"""The transaction signature hash (zg_tx_layout, zg_sighash), CPU tier.

  * tests/sighash_ref.py against every vector of tests/golden/sighash.json (the fixture generator asserted the
    same restatement against all 500 of the reference's vectors);
  * zg_tx_layout: counts of every fixture transaction, every proper prefix, trailing bytes, a wrong version
    group, a count of 2^32, every compact size in each non-minimal form;
  * the hashing routine the kernels run, compiled for the host (tests/native/zg_hosttest_sighash.hip), against
    the fixture and the synthesized case lists of tests/sighash_cases.py;
  * the same source as a stand-alone program under the address and undefined-behaviour sanitizers: the prefix
    sweep and the fixture hashes over heap blocks of exactly the input's size."""
import shutil
import subprocess

import pytest

from tests import sighash_cases as C
from tests import sighash_ref as R
from tests.conftest import load_golden
from zebra_amd import zg

needs_hipcc = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")


# ------------------------------------------------------------------ the restatement
def test_reference_restatement_matches_every_fixture_vector():
    g = load_golden("sighash.json")
    assert len(g["vectors"]) >= 32 and len(g["sapling_spends"]) == 2 and len(g["legacy"]) == 5
    classes = set()
    for v in g["vectors"] + g["sapling_spends"]:
        raw = bytes.fromhex(v["tx"])
        got = R.sighash(raw, v["input_index"], bytes.fromhex(v["script"]), v["amount"], v["hashtype"], v["branch_id"])
        assert got == (bytes.fromhex(v["sighash"]), R.SIGHASH_OK)
        classes.add((R.parse(raw)[1]["sigver"], R._base(v["hashtype"]), bool(v["hashtype"] & 0x80)))
    assert len(classes) == 17
    txs, br, items, expected = C.fixture_cases()
    assert R.run(txs, br, items) == ([R.TX_OK] * len(txs), expected, [R.SIGHASH_OK] * len(items))


def test_the_sapling_era_spends_need_their_amount():
    from tests import ecdsa_ref as E
    for v in load_golden("sighash.json")["sapling_spends"]:
        raw, code = bytes.fromhex(v["tx"]), bytes.fromhex(v["script"])
        pk, sig = bytes.fromhex(v["pubkey"]), bytes.fromhex(v["sig"])
        assert E.verify(pk, sig, R.sighash(raw, 0, code, v["amount"], v["hashtype"], v["branch_id"])[0]) == E.OK
        assert E.verify(pk, sig, R.sighash(raw, 0, code, 0, v["hashtype"], v["branch_id"])[0]) == E.SIGNATURE


# ------------------------------------------------------------------ zg_tx_layout
def test_layout_of_every_fixture_transaction():
    txs, _, _, _ = C.fixture_cases()
    assert {zg.tx_layout(t)[1][6] for t in txs} == {0, 1, 2}
    for t in txs:
        assert zg.tx_layout(t) == R.layout(t) and zg.tx_layout(t)[0] == zg.TX_OK


def test_layout_of_synthesized_transactions():
    for name in C.SYNTHESIZED:
        for t in C.SYNTHESIZED[name]()[0]:
            assert zg.tx_layout(t) == R.layout(t), name
    st, out = zg.tx_layout(C.make_tx("sapling", 253, 253, n_js=2, n_spend=3, n_sout=4))
    assert (st, out[1:7]) == (zg.TX_OK, [253, 253, 2, 3, 4, 2])


def test_every_proper_prefix_is_malformed():
    for t in C.small_txs() + [C.make_tx("sapling", 1, 1, n_js=1, n_spend=1, n_sout=1), C.make_tx("v2", 1, 1, n_js=1)]:
        assert zg.tx_layout(t)[0] == zg.TX_OK
        for k in range(len(t)):
            assert zg.tx_layout(t[:k]) == (zg.TX_MALFORMED, [0] * 8), k


def test_trailing_byte_and_wrong_version_group_are_malformed():
    for t in C.small_txs():
        assert zg.tx_layout(t + b"\x00")[0] == zg.TX_MALFORMED
    ow, sap = C.small_txs()[1:]
    for t, header, vgid in ((ow, 0x80000003, R.SAPLING_VGID), (sap, 0x80000004, R.OVERWINTER_VGID),
                            (ow, 0x80000002, R.OVERWINTER_VGID), (sap, 0x80000005, R.SAPLING_VGID),
                            (sap, 0x80000004, R.SAPLING_VGID ^ 1)):
        bad = header.to_bytes(4, "little") + vgid.to_bytes(4, "little") + t[8:]
        assert zg.tx_layout(bad)[0] == zg.TX_MALFORMED == R.layout(bad)[0]
    assert zg.tx_layout(b"\x05\x00\x00\x00" + C.small_txs()[0][4:])[0] == zg.TX_OK   # not overwintered: any version


def test_a_count_of_2_to_the_32_is_malformed():
    big = b"\xff" + (1 << 32).to_bytes(8, "little")
    for body in (b"\x01\x00\x00\x00" + big, b"\x01\x00\x00\x00\x00" + big,
                 (0x80000004).to_bytes(4, "little") + R.SAPLING_VGID.to_bytes(4, "little") + b"\x00\x00" + bytes(16) + big):
        for tail in (b"", bytes(100)):
            assert zg.tx_layout(body + tail) == (zg.TX_MALFORMED, [0] * 8) == R.layout(body + tail)


def test_every_non_minimal_compact_size_is_noncanonical():
    kw = dict(n_js=1, n_spend=1, n_sout=1, seed=9)
    assert zg.tx_layout(C.make_tx("sapling", 2, 2, **kw))[0] == zg.TX_OK
    for tag in C.COMPACT_TAGS:
        for form in (0xFD, 0xFE, 0xFF):
            t = C.make_tx("sapling", 2, 2, enc={tag: C.long_form(form)}, **kw)
            st, out = zg.tx_layout(t)
            assert st == zg.TX_NONCANONICAL and out[1:8] == [2, 2, 1, 1, 1, 2, len(t)], (tag, form)
            assert (st, out) == R.layout(t)
            assert zg.tx_layout(t[:-1])[0] == zg.TX_MALFORMED      # MALFORMED wins
    # the long forms are fine where they are the shortest
    t = C.make_tx("v2", 253, 1, max_script=300, seed=3)
    assert zg.tx_layout(t) == R.layout(t) and zg.tx_layout(t)[0] == zg.TX_OK
    assert zg.tx_layout(b"")[0] == zg.TX_MALFORMED


# ------------------------------------------------------------------ the kernels' routine on the host
@needs_hipcc
def test_host_build_matches_every_fixture_vector():
    from tests import sighash_hostlib as H
    txs, br, items, expected = C.fixture_cases()
    assert H.sighash(txs, br, items) == ([0] * len(txs), expected, [0] * len(items))
    assert H.sighash(txs, br, items, threads=4)[1] == expected


@needs_hipcc
@pytest.mark.parametrize("name", sorted(C.SYNTHESIZED))
def test_host_build_matches_the_synthesized_cases(name):
    from tests import sighash_hostlib as H
    txs, br, items, want = C.case(name)
    assert H.sighash(txs, br, items, threads=8) == want
    if name == "status_plumbing":
        assert sorted(set(want[2])) == [0, 1, 2] and want[0] == [0, 1, 0, 2, 0]
    if name == "sapling_edges":
        assert 3 in want[2]
    if name == "sprout_edges":
        assert want[1].count(R.ZERO) >= 16 and set(want[2]) == {0}


@needs_hipcc
def test_standalone_program_under_sanitizers(tmp_path):
    """parser and hasher over exact-size heap blocks: the prefix sweep of five transactions, every fixture
    vector, the count edges and the status cases"""
    from tests import sighash_hostlib as H
    exe = H.build_program(str(tmp_path / "zg_hosttest_sighash"))
    lines, swept = [], set()

    def add(txs, br, items, hashes, statuses):
        for (t, idx, code, amount, ht), h, st in zip(items, hashes, statuses):
            sweep = len(txs[t]) < 4000 and txs[t] not in swept     # every proper prefix, once per transaction
            swept.add(txs[t])
            lines.append("%s %s %d %d %d %d %s %d %d" % (
                txs[t].hex() or "-", code.hex() or "-", -1 if idx is None else idx, amount, ht, br[t], h.hex(), st,
                sweep))

    txs, br, items, expected = C.fixture_cases()
    add(txs, br, items, expected, [0] * len(items))
    for name in ("count_edges", "sprout_edges", "sapling_edges", "status_plumbing"):
        txs, br, items, want = C.case(name)
        picked = range(0, len(items), 5)
        add(txs, br, [items[k] for k in picked], [want[1][k] for k in picked], [want[2][k] for k in picked])
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    last = r.stdout.strip().splitlines()[-1].split()
    assert last[0] == "cases" and int(last[1]) == len(lines) and int(last[3]) == 0
    assert int(last[5]) > 5000 and int(last[7]) == 0          # every proper prefix swept was MALFORMED


# ------------------------------------------------------------------ the collector (reference backends, no GPU)
def reference_backends(calls=None):
    from oracle import sapling_sig as S
    from tests import ecdsa_ref as E, ed25519_ref as ED

    def sighash(txs, br, items):
        if calls is not None:
            calls.append(len(items))
        return R.run(txs, br, items)
    return dict(
        verify=lambda proofs, kinds, inputs, n_inputs: [0] * len(kinds), sighash=sighash,
        verify_ecdsa=lambda pk, sg, m: [E.verify(a, b, c) for a, b, c in zip(pk, sg, m)],
        verify_js_sigs=lambda pk, sg, m: [ED.verify(a, b, c) for a, b, c in zip(pk, sg, m)],
        verify_sigs=lambda vk, sg, m, gen: [S.redjubjub_verify(a, b, c, d) for a, b, c, d in zip(vk, sg, m, gen)],
        sapling_bvk=lambda txs: [(0, S.encode(S.binding_verification_key(sp, ou, vb))) for sp, ou, vb in txs])


def test_collector_resolves_raw_transactions_and_requests():
    from tests.test_gpu_sighash import window
    from zebra_amd.collector import verify_block
    calls = []
    kw = reference_backends(calls)
    assert verify_block(window("host"), **kw) is None and calls == []      # neither new field: no sighash call
    assert verify_block(window("raw"), **kw) is None and len(calls) == 1   # ONE call for the window
    for k in (0, 1):
        want = (k, ("Signature", k, "EvalFalse"))
        assert verify_block(window("host", bump_amount=k), **kw) == want == verify_block(window("raw", bump_amount=k), **kw)
    w = window("raw")
    w[-1].branch_id ^= 1
    assert verify_block(w, **kw) == (len(w) - 1, "JoinSplitSignature")
    # the input list is not modified
    w = window("raw")
    verify_block(w, **kw)
    assert all(t.sighash is None and not t.ecdsa_checks for t in w)


def test_collector_rerun_lookup_by_request_and_explicit_errors():
    from tests.test_gpu_sighash import window
    from zebra_amd.collector import verify_block
    g = load_golden("sighash.json")
    calls = []
    kw = reference_backends(calls)
    w = window("raw", bump_amount=0)
    req = w[0].ecdsa_requests[0]
    good = g["sapling_spends"][0]
    seen = []

    def rerun(lookup):
        # the recorded request, by its key: in the window's table, no further sighash call
        seen.append(lookup(req.input_index, req.pubkey, req.sig, req.script_code, req.hashtype))
        n = len(calls)
        seen.append(lookup(req.input_index, req.pubkey, req.sig, req.script_code, req.hashtype))
        assert len(calls) == n
        # another script code for the same input (as OP_CHECKMULTISIG or a code separator would ask): one further call
        seen.append(lookup(req.input_index, req.pubkey, req.sig, req.script_code + b"\x00", req.hashtype))
        assert calls[-1] == 1 and len(calls) == n + 1
        return ("Signature", 0, "EvalFalse")
    w[0].eval_rerun = rerun
    assert verify_block(w, **kw) == (0, ("Signature", 0, "EvalFalse")) and seen == [False, False, False]
    assert good["amount"] + 1 == req.amount
    # a transaction the parser does not pass is the caller's: never accepted silently
    for breakage in (lambda raw: raw[:-1], lambda raw: raw + b"\x00"):
        w = window("raw")
        w[2].raw = breakage(w[2].raw)
        with pytest.raises(zg.ZgError, match="transaction 2"):
            verify_block(w, **kw)
    w = window("raw")
    w[1].ecdsa_requests[0].input_index = 99            # ZG_SIGHASH_INPUT_RANGE
    with pytest.raises(zg.ZgError, match="transaction 1"):
        verify_block(w, **kw)
    w = window("raw")
    w[0].raw = None
    with pytest.raises(zg.ZgError):
        verify_block(w, **kw)
    w = window("raw")
    del kw["sighash"]
    with pytest.raises(zg.ZgError):
        verify_block(w, **kw)
