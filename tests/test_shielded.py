"""CPU tier of zg_shielded_verify: the oracle on the real transactions, the host build of the plan,
gather, row and fold routines against it on every case, the stand-alone program under sanitizers, the device's
JoinSplit preparation against zg_prep_joinsplit, the ABI, the kernels' resources and the collector's opt-in."""
import shutil
import subprocess
import tempfile

import pytest

from tests import shielded_cases as C
from tests import shielded_ref as S
from zebra_amd import zg

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")

# kernel -> (VGPR ceiling, scratch bytes per lane, LDS bytes): the figures of profiles/f17_shielded_resource_usage.txt
CEILINGS = {"k_shd_gather": (112, 0, 0), "k_shd_rows": (40, 0, 0), "k_shd_descs": (10, 0, 0), "k_shd_fold": (12, 0, 0)}


@pytest.fixture(scope="module")
def want():
    cs = C.cases()
    return S.run([c[1] for c in cs], [c[2] for c in cs])


# ------------------------------------------------------------------ the oracle
def test_oracle_passes_the_real_transactions(want):
    names = [c[0] for c in C.cases()]
    for k in C.SIX + ("transparent",):
        i = names.index(k)
        assert (want[0][i], want[1][i], want[2][i], want[3][i]) == (0, S.SHTX_OK, 0, 0), k
        assert want[4][i] != S.ZERO and set(want[5][i]) <= {0}
    from tests.conftest import load_golden
    g = load_golden("sighash.json")
    for i, v in enumerate(g["sapling"]):
        assert want[4][names.index("sap%d" % i)].hex() == v["sighash"]
    for i, v in enumerate(g["joinsplit"]):
        assert want[4][names.index("js%d" % i)].hex() == v["sighash"]


def test_oracle_default_binding_signature():
    """a v4 transaction without spends and outputs: accept_sapling_final on 64 zero bytes and bvk = -[vb] G_v"""
    from oracle import sapling_sig
    h = bytes(range(32))
    assert sapling_sig.binding_sig_ok([], [], 0, h, bytes(64))
    assert not sapling_sig.binding_sig_ok([], [], 5, h, bytes(64))
    assert not sapling_sig.binding_sig_ok([], [], -595, h, bytes(64))


def test_case_list_covers_every_class(want):
    """the list, not a tolerance, is the condition: every ZG_SHTX_* and every reachable ZG_SHD_* occurs"""
    assert set(want[1]) == set(range(8))
    seen = set(want[3]) | {d for row in want[5] for d in row}
    assert seen == set(range(20)) - set(S.SHD_UNREACHABLE)
    names = [c[0] for c in C.cases()]
    # precedence: a flipped spend proof byte lies under the hash, so the spend-auth class comes first
    i = names.index("spend_proof_byte")
    assert (want[1][i], want[3][i]) == (S.SHTX_INVALID_SAPLING, S.SHD_SPEND_AUTH_SIG)
    i = names.index("spend_own_key")
    assert (want[1][i], want[3][i]) == (S.SHTX_INVALID_SAPLING, S.SHD_PROOF_FAILED)
    i = names.index("ciphertext_byte")
    assert (want[3][i], want[5][i]) == (S.SHD_BINDING_SIGNATURE, [0])
    i = names.index("js_own_key")
    assert (want[1][i], want[2][i], want[3][i]) == (S.SHTX_INVALID_JOINSPLIT, 0, S.SHD_JOINSPLIT_PROOF)


# ------------------------------------------------------------------ the host build
def host_run(cs):
    from tests import shielded_hostlib as H
    txs, br = [c[1] for c in cs], [c[2] for c in cs]
    parts = [S.parts(raw, b) if S.verify_tx(raw, b)[1] in (S.SHTX_OK, S.SHTX_JOINSPLIT_SIGNATURE, S.SHTX_INVALID_JOINSPLIT,
                                                          S.SHTX_INVALID_SAPLING) else None for raw, b in zip(txs, br)]
    zero = {"hash": bytes(32), "bvk": bytes(32), "bvk_st": 0, "bind_ok": 0, "ed": 0, "descs": []}
    per = [p or zero for p in parts]
    descs = [d for p in per for d in p["descs"]]
    got = H.shielded_verify(txs, br, [p["hash"] for p in per], [p["bvk"] for p in per], [p["bvk_st"] for p in per],
                            [p["bind_ok"] for p in per], [p["ed"] for p in per], [d[4] for d in descs],
                            [d[5] for d in descs])
    return got, parts, descs


def test_host_build_matches_the_oracle(want):
    got, parts, descs = host_run(C.cases())
    names = [c[0] for c in C.cases()]
    for k, what in enumerate(("tx_status", "status", "index", "detail")):
        assert got[what] == want[k], [(n, a, b) for n, a, b in zip(names, got[what], want[k]) if a != b]
    assert got["desc_status"] == want[5]
    # the gathered rows: kinds, proofs, preparation classes and public inputs, the device-written input counts
    assert got["kinds"] == [d[0] for d in descs] and got["proofs"] == [d[1] for d in descs]
    assert got["codes"] == [d[2] for d in descs] and got["inputs"] == [d[3] for d in descs]
    assert got["ninputs"] == [0 if d[2] else {0: 7, 1: 5, 2: 9}[d[0]] for d in descs]
    live = [p for p in parts if p]
    assert got["rj"] == [r for p in live for r in p["rj_spends"]] + [p["rj_binding"] for p in live]
    assert got["ed"] == [p["ed_row"] for p in live if p["ed_row"]]
    assert got["counts"] == (len(descs), len(got["rj"]), len(got["ed"]), len(live))


@pytest.mark.parametrize("make", [C.spliced_outputs, C.spliced_joinsplits, C.spliced_spends])
def test_host_build_spliced_positions(make):
    pos = (0, 63, 64, 129)
    cs = [("", make(130, j), C.SAPLING_BRANCH) for j in pos]
    got, _, _ = host_run(cs)
    w = S.run([c[1] for c in cs], [c[2] for c in cs])
    assert (got["status"], got["index"], got["detail"], got["desc_status"]) == (w[1], w[2], w[3], w[5])
    for j, row in zip(pos, got["desc_status"]):
        assert row[j] != 0


def test_host_build_empty_window():
    from tests import shielded_hostlib as H
    got = H.shielded_verify([], [], [], [], [], [], [], [], [])
    assert got["counts"] == (0, 0, 0, 0) and got["status"] == []


def test_device_joinsplit_preparation_is_zg_prep_joinsplit():
    """hSig in one BLAKE2b block and the byte-window packing, against the public host function and the oracle"""
    from oracle import zcash
    from tests import shielded_hostlib as H
    from tests import sighash_ref as R
    n = 0
    for name, raw, _ in C.cases():
        st, t = R.parse(raw)
        if st != 0 or t["sigver"] != 2:
            continue
        for d in t["joinsplits"]:
            desc, _ = S.joinsplit_fields(d)
            row = H.prep_joinsplit(d, t["js_pubkey"])
            ref = zg.prep_joinsplit(desc["anchor"], desc["random_seed"], desc["nullifiers"], desc["macs"],
                                    desc["commitments"], desc["vpub_old"], desc["vpub_new"], t["js_pubkey"])
            assert row == b"".join(ref), name
            assert [int.from_bytes(row[32 * j:32 * j + 32], "little") for j in range(9)] == \
                zcash.sprout_inputs(desc, t["js_pubkey"]), name
            n += 1
    assert n >= 12


def test_standalone_program_under_sanitizers(tmp_path):
    """every case and every proper prefix of it, in heap blocks of exactly their sizes"""
    from tests import shielded_hostlib as H
    exe = H.build_program(str(tmp_path / "zg_hosttest_shielded"))
    cs = C.cases()
    path = tmp_path / "cases.txt"
    path.write_text("".join("%x %s\n" % (b, raw.hex()) for _, raw, b in cs))
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.split()[0] == str(len(cs))


# ------------------------------------------------------------------ the ABI and the kernels
def test_abi_exports_and_constants():
    L = zg.lib()
    assert hasattr(L, "zg_shielded_verify") and hasattr(zg.Context, "shielded_verify")
    hdr = open(zg.HERE + "/../include/zg.h").read()
    for k in dir(S):
        if k.startswith(("SHTX_", "SHD_")) and isinstance(getattr(S, k), int):
            assert "#define ZG_%s %d" % (k, getattr(S, k)) in hdr and getattr(zg, k) == getattr(S, k), k
    assert zg.pack_shielded([b"ab", b"c"], [1, 2])[0] == b"abc"


def test_shielded_kernels_stay_in_registers():
    from tools import resource_table
    with tempfile.TemporaryDirectory() as tmp:
        rows = {r["name"]: r for r in resource_table.unit("zg_shielded.hip", tmp) if "occ" in r}
    assert len(rows) == len(CEILINGS), sorted(rows)
    for part, (vgpr, scratch, lds) in CEILINGS.items():
        (name, r), = [(n, r) for n, r in rows.items() if part in n]
        assert r["vgpr"] <= vgpr and r["scratch"] <= scratch and r["lds"] <= lds, (name, r)
        assert r.get("vspill", 0) == 0 and r.get("sspill", 0) == 0 and r["occ"] >= 2, (name, r)


# ------------------------------------------------------------------ the collector, with a stand-in verifier
def test_collector_opt_in_one_call_and_precedence():
    from zebra_amd.collector import Tx, verify_block
    calls = []

    def backend(txs, branch_ids):
        calls.append(len(txs))
        return S.run(txs, branch_ids)
    cs = {c[0]: c for c in C.cases()}
    tx = lambda name, **kw: Tx(raw=cs[name][1], branch_id=cs[name][2], shielded=True, **kw)  # noqa: E731
    kw = dict(verify=lambda *a: [], shielded_verify=backend)
    ok = [tx("sap0"), tx("js0"), tx("transparent"), tx("v1")]
    assert verify_block(ok, **kw) is None and calls == [4]
    assert verify_block(ok + [tx("spend_own_key")], **kw) == (4, "InvalidSapling")
    assert verify_block(ok + [tx("js_sig_bit")], **kw) == (4, "JoinSplitSignature")
    assert verify_block(ok + [tx("js_own_key")], **kw) == (4, ("InvalidJoinSplit", 0))
    # the caller's outcomes keep their places: a tree error after its own description's proof, before a later one's
    assert verify_block([tx("joinsplits3_foreign2", tree_errors=[None, "UnknownAnchor"])], **kw) == (0, "JoinSplitSignature")
    own = C.build(C.own_joinsplit_key(dict(C.parsed(C.real()["js0"]), joinsplits=[
        C.parsed(C.real()["js0"])["joinsplits"][0]] * 3)))
    t = lambda **k: Tx(raw=own, branch_id=C.SAPLING_BRANCH, shielded=True, **k)  # noqa: E731
    assert verify_block([t()], **kw) == (0, ("InvalidJoinSplit", 0))
    cs3 = C.build(C.own_joinsplit_key(dict(C.parsed(C.real()["js0"]))))
    assert S.verify_tx(cs3, C.SAPLING_BRANCH)[1] == S.SHTX_INVALID_JOINSPLIT
    good = lambda **k: Tx(raw=cs["js0"][1], branch_id=C.SAPLING_BRANCH, shielded=True, **k)  # noqa: E731
    assert verify_block([good(tree_errors=["UnknownAnchor"])], **kw) == (0, "UnknownAnchor")
    assert verify_block([good(js_nullifier_error="JoinSplitDeclared")], **kw) == (0, "JoinSplitDeclared")
    assert verify_block([tx("js_own_key", tree_errors=["UnknownAnchor"])], **kw) == (0, ("InvalidJoinSplit", 0))
    assert verify_block([tx("sap0", sapling_nullifier_error="SaplingDeclared")], **kw) == (0, "SaplingDeclared")
    assert verify_block([tx("binding_sig_bit", sapling_nullifier_error="SaplingDeclared")], **kw) == (0, "InvalidSapling")
    assert verify_block([tx("js_and_sapling", js_nullifier_error="JoinSplitDeclared")], **kw) == (0, "JoinSplitSignature")
    assert verify_block([tx("sap0", pre_error="Maturity")], **kw) == (0, "Maturity")
    with pytest.raises(zg.ZgError):
        verify_block([tx("v3_host")], **kw)
    with pytest.raises(ValueError):
        verify_block([tx("sap0", sighash=bytes(32))], **kw)
    with pytest.raises(ValueError):
        verify_block([Tx(shielded=True)], **kw)
    # without the mark nothing goes to the new backend
    n = len(calls)
    assert verify_block([Tx()], **kw) is None and len(calls) == n
