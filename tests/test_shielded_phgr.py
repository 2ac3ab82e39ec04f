"""CPU tier of zg_shielded_verify_flags with ZG_SHIELDED_PHGR: the fixture against the oracle's parts,
the host build of the PHGR plan, gather, row and fold routines against tests/shielded_phgr_ref.py on every case, the
stand-alone program under sanitizers, the ABI and its argument checks, the kernels' resources and the collector's
option."""
import ctypes
import shutil
import subprocess
import tempfile

import pytest

from tests import shielded_cases as C4
from tests import shielded_phgr_cases as C
from tests import shielded_phgr_ref as P
from tests import shielded_ref as S
from tests.conftest import load_golden
from zebra_amd import zg

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")

PHGR = P.SHIELDED_PHGR
# kernel -> (VGPR ceiling, scratch bytes per lane, LDS bytes). The rows and fold kernels: the ceilings of their f17
# neighbours (k_shd_rows 40, k_shd_fold 12). The gather: 128, the most that keeps k_shd_gather's four waves per SIMD
# (512 / 128). profiles/f18_shielded_phgr_resource_usage.txt has the figures: 118, 38 and 11.
CEILINGS = {"k_shp_gather": (128, 0, 0), "k_shp_rows": (40, 0, 0), "k_shp_fold": (12, 0, 0)}


def by_name(cs, want):
    names = [c[0] for c in cs]
    return lambda k: tuple(want[j][names.index(k)] for j in range(6))


@pytest.fixture(scope="module")
def want():
    cs = C.cases()
    return P.run([c[1] for c in cs], [c[2] for c in cs], PHGR)


# ------------------------------------------------------------------ the fixture and the reference
def test_fixture_is_what_the_references_give():
    g = load_golden("phgr_txs.json")
    assert len(g["txs"]) == 5 and sum(len(t["joinsplits"]) for t in g["txs"]) == 6
    known = {(c["proof"], tuple(c["inputs"])): c["status"] for c in load_golden("pghr13.json")["cases"]}
    for t in g["txs"]:
        raw = bytes.fromhex(t["raw"])
        p = P.parts(raw, 0)
        assert p["hash"].hex() == t["sighash"] and p["ed"] == t["ed25519"] == 0
        assert [d[2] for d in p["descs"]] == t["joinsplits"] == [0] * len(p["descs"])
        for proof, inputs in P.pairs(raw):
            assert known[(proof.hex(), P.fr_hex(inputs))] == 0
    # every pair the cases use is recorded: no test runs the Python pairing
    rec = {(v["proof"], tuple(v["inputs"])) for v in g["verdicts"]}
    for raw in C.every_tx() + [c[1] for c in C.interleaved_cases()]:
        for proof, inputs in P.pairs(raw):
            assert (proof.hex(), P.fr_hex(inputs)) in rec


def test_reference_classes(want):
    """the list, not a tolerance, is the condition: every class a transaction before v4 can have occurs, at the
    places the reference's order gives them"""
    get = by_name(C.cases(), want)
    for i in range(5):
        st = get("real%d" % i)
        assert st[:4] == (0, S.SHTX_OK, 0, 0) and set(st[5]) == {0}
        assert st[4].hex() == load_golden("phgr_txs.json")["txs"][i]["sighash"]
    # the signature covers the proof: a changed proof is a signature failure first; desc_status shows the description
    assert get("proof_byte_1")[1:4] == (S.SHTX_JOINSPLIT_SIGNATURE, 0, S.SHD_ED_SIGNATURE)
    assert get("proof_byte_1")[5] == [S.SHD_OK, P.SHD_JOINSPLIT_PGHR_PROOF]
    for name, _, _ in C.encoding_mutants():
        assert get("encoding_1_" + name)[1] == S.SHTX_JOINSPLIT_SIGNATURE
        assert get("encoding_1_" + name)[5] == [S.SHD_OK, S.SHD_JOINSPLIT_ENCODING]
    assert get("own_key")[1:4] == (S.SHTX_INVALID_JOINSPLIT, 0, P.SHD_JOINSPLIT_PGHR_PROOF)
    assert get("own_key")[5] == [P.SHD_JOINSPLIT_PGHR_PROOF] * 2
    for name, _, _ in C.encoding_mutants()[:2]:
        st = get("own_key_encoding_0_" + name)
        assert st[1:4] == (S.SHTX_INVALID_JOINSPLIT, 0, S.SHD_JOINSPLIT_ENCODING)
        assert st[5] == [S.SHD_JOINSPLIT_ENCODING, P.SHD_JOINSPLIT_PGHR_PROOF]
    assert get("ed_pubkey_invalid")[1:4] == (S.SHTX_JOINSPLIT_SIGNATURE, 0, S.SHD_ED_PUBLIC_ENCODING)
    assert get("ed_sig_s_high")[1:4] == (S.SHTX_JOINSPLIT_SIGNATURE, 0, S.SHD_ED_SIGNATURE_ENCODING)
    assert get("ed_sig_bit")[1:4] == (S.SHTX_JOINSPLIT_SIGNATURE, 0, S.SHD_ED_SIGNATURE)
    # v3: the ZIP-143 digest, under which the Sprout-form signature does not hold; the proofs do not depend on it
    v3 = get("v3_same_signature")
    assert v3[1:4] == (S.SHTX_JOINSPLIT_SIGNATURE, 0, S.SHD_ED_SIGNATURE) and v3[5] == [0, 0]
    assert v3[4] != get("real4")[4] and v3[4] == C.sighash(C.overwinter(C.two()))
    assert get("v3_own_key")[1:4] == (S.SHTX_INVALID_JOINSPLIT, 0, P.SHD_JOINSPLIT_PGHR_PROOF)


def test_reference_without_the_flag_is_the_f17_reference():
    cs = C.interleaved_cases()
    txs, br = [c[1] for c in cs], [c[2] for c in cs]
    off, on = P.run(txs, br, 0), P.run(txs, br, PHGR)
    assert off == S.run(txs, br)
    for t, c in enumerate(cs):
        if off[1][t] == S.SHTX_HOST:
            assert (off[2][t], off[3][t], off[4][t], off[5][t]) == (0, 0, S.ZERO, [])
            assert on[1][t] != S.SHTX_HOST and on[4][t] != S.ZERO and on[5][t], c[0]
        else:
            assert tuple(on[k][t] for k in range(6)) == tuple(off[k][t] for k in range(6)), c[0]
    assert S.SHTX_HOST not in on[1] and off[1].count(S.SHTX_HOST) == len(C.cases()) + 1
    with pytest.raises(ValueError):
        P.run(txs[:1], br[:1], 2)


# ------------------------------------------------------------------ the host build
def host_run(txs, br, flags=PHGR):
    from tests import shielded_phgr_hostlib as H
    ref = [P.verify_tx(raw, b, flags) for raw, b in zip(txs, br)]
    live = (S.SHTX_OK, S.SHTX_JOINSPLIT_SIGNATURE, S.SHTX_INVALID_JOINSPLIT, S.SHTX_INVALID_SAPLING)
    zero = {"hash": bytes(32), "bvk": bytes(32), "bvk_st": 0, "bind_ok": 0, "ed": 0, "descs": []}
    v4, pg = [], []
    for (raw, b), r in zip(zip(txs, br), ref):
        sap = r[0] == 0 and C.R.parse(raw)[1]["sigver"] == 2
        v4.append(S.parts(raw, b) if sap and r[1] in live else None)
        pg.append(P.parts(raw, b) if not sap and r[1] in live else None)
    per = [a or dict(zero, **(p or {})) for a, p in zip(v4, pg)]
    d4 = [d for a in v4 if a for d in a["descs"]]
    dp = [d for p in pg if p for d in p["descs"]]
    rc, got = H.shielded_verify(txs, br, flags, [p["hash"] for p in per], [p.get("bvk", bytes(32)) for p in per],
                                [p.get("bvk_st", 0) for p in per], [p.get("bind_ok", 0) for p in per],
                                [p["ed"] for p in per], [d[4] for d in d4], [d[5] for d in d4], [d[2] for d in dp])
    assert rc == 0
    return got, ref, v4, pg, d4, dp


def check_host(txs, br, flags=PHGR, names=None):
    got, ref, v4, pg, d4, dp = host_run(txs, br, flags)
    for k, what in enumerate(("tx_status", "status", "index", "detail")):
        assert got[what] == [r[k] for r in ref], [(names[t] if names else t, a, r[k])
                                                  for t, (a, r) in enumerate(zip(got[what], ref)) if a != r[k]]
    assert got["desc_status"] == [r[5] for r in ref]
    # the gathered PHGR rows: the proofs as they lie in the transactions, the inputs as Input::into_bn_frs gives them
    assert got["pg_proofs"] == [d[0] for d in dp] and got["pg_inputs"] == [d[1] for d in dp]
    assert got["proofs"] == [d[1] for d in d4]
    # the Ed25519 rows: the v4 transactions' first, then those before v4
    assert got["ed"] == [a["ed_row"] for a in v4 if a and a["ed_row"]] + [p["ed_row"] for p in pg if p]
    n4, npg = sum(1 for a in v4 if a), sum(1 for p in pg if p)
    assert got["counts"][0] == len(d4) and got["counts"][2:] == (len(got["ed"]), n4, npg, len(dp))
    return got


def test_host_build_matches_the_reference():
    cs = C.cases()
    check_host([c[1] for c in cs], [c[2] for c in cs], PHGR, [c[0] for c in cs])


def test_host_build_interleaved_with_the_f17_cases():
    cs = C.interleaved_cases()
    got = check_host([c[1] for c in cs], [c[2] for c in cs], PHGR, [c[0] for c in cs])
    assert S.SHTX_HOST not in got["status"]
    assert 20 in {d for row in got["desc_status"] for d in row}


def test_host_build_without_the_flag_and_unknown_flags():
    from tests import shielded_phgr_hostlib as H
    cs = C.interleaved_cases()
    txs, br = [c[1] for c in cs], [c[2] for c in cs]
    got = check_host(txs, br, 0)
    assert got["counts"][4:] == (0, 0) and got["status"].count(S.SHTX_HOST) == len(C.cases()) + 1
    n = len(txs)
    rc, _ = H.shielded_verify(txs, br, 2, [bytes(32)] * n, [bytes(32)] * n, bytes(n), bytes(n), bytes(n), b"", b"", b"")
    assert rc == -2


def test_host_build_spliced_positions():
    pos = (0, 63, 64, 129)
    txs = [C.spliced(130, j) for j in pos]
    got = check_host(txs, [0] * 4)
    for j, row in zip(pos, got["desc_status"]):
        assert row == [P.SHD_JOINSPLIT_PGHR_PROOF if i == j else 0 for i in range(130)]
    assert set(got["status"]) == {S.SHTX_JOINSPLIT_SIGNATURE}


@pytest.mark.parametrize("n_phgr", [1, 63, 64, 65, 130])
def test_host_build_mixed_windows(n_phgr):
    txs, br = C.mixed_window(n_phgr)
    got = check_host(txs, br)
    assert got["counts"][0] == 65 and got["counts"][5] == n_phgr
    pg = [row for raw, row in zip(txs, got["desc_status"]) if C.R.parse(raw)[1]["sigver"] != 2]
    assert pg[0][0] == P.SHD_JOINSPLIT_PGHR_PROOF and pg[-1][-1] == P.SHD_JOINSPLIT_PGHR_PROOF
    assert sum(len(r) for r in pg) == n_phgr and sum(1 for r in pg for c in r if c) == min(n_phgr, 2)


def test_host_build_phgr_only_and_v4_only_windows():
    got = check_host(C.phgr_window(5), [0] * len(C.phgr_window(5)))
    assert got["counts"][:2] == (0, 0) and got["counts"][3] == 0 and got["counts"][5] == 5
    txs, br = C4.window(10)
    on, off = check_host(txs, br, PHGR), check_host(txs, br, 0)
    assert on == off and on["counts"][4:] == (0, 0)


@pytest.mark.parametrize("lead", [0, 1, 2, 3])
def test_host_build_every_alignment(lead):
    cs = C.cases()
    txs, br = [bytes(lead)] + [c[1] for c in cs], [0] + [c[2] for c in cs]
    got = check_host(txs, br)
    assert got["status"][0] == S.SHTX_TX_MALFORMED


def test_standalone_program_under_sanitizers(tmp_path):
    """every case and every proper prefix of it, in heap blocks of exactly their sizes; the 130-description
    transactions whole (their prefixes add nothing to those of the two-description case but minutes)"""
    from tests import shielded_phgr_hostlib as H
    exe = H.build_program(str(tmp_path / "zg_hosttest_shielded_phgr"))
    cs = C.cases()
    lines = ["%x %s\n" % (b, raw.hex()) for _, raw, b in cs]
    lines += ["=0 %s\n" % C.spliced(130, j).hex() for j in (0, 129)]
    lines += ["%x %s\n" % (c[2], c[1].hex()) for c in C4.cases()[:8]]
    path = tmp_path / "cases.txt"
    path.write_text("".join(lines))
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.split()[0] == str(len(lines))


# ------------------------------------------------------------------ the ABI and the kernels
def test_abi_exports_constants_and_bindings():
    L = zg.lib()
    assert hasattr(L, "zg_shielded_verify_flags")
    hdr = open(zg.HERE + "/../include/zg.h").read()
    assert "#define ZG_SHD_JOINSPLIT_PGHR_PROOF 20" in hdr and zg.SHD_JOINSPLIT_PGHR_PROOF == P.SHD_JOINSPLIT_PGHR_PROOF == 20
    assert "#define ZG_SHIELDED_PHGR 1u" in hdr and zg.SHIELDED_PHGR == PHGR == 1
    import inspect
    assert inspect.signature(zg.Context.shielded_verify).parameters["phgr"].default is False
    from zebra_amd import collector
    assert inspect.signature(collector.verify_block).parameters["shielded_phgr"].default is False
    ffi = open(zg.HERE + "/../rust/verification/src/gpu/ffi.rs").read()
    assert "pub fn zg_shielded_verify_flags(" in ffi and "pub const ZG_SHIELDED_PHGR: u32 = 1;" in ffi


def test_entry_rejects_bad_arguments_before_the_device():
    """an unknown flag bit and the argument checks of zg_shielded_verify: ZG_E_INVAL with no context touched"""
    L = zg.lib()
    one = ctypes.create_string_buffer(64)
    off = (ctypes.c_uint64 * 2)(0, 4)
    br = (ctypes.c_uint32 * 1)(0)
    ix = (ctypes.c_uint64 * 1)()
    f = L.zg_shielded_verify_flags
    assert f(None, 0, None, None, None, PHGR, None, None, None, None, None, None, None) == -1
    # a context pointer is not followed when the flags are wrong: the check comes with the argument checks
    fake = ctypes.cast(ctypes.create_string_buffer(1 << 16), ctypes.c_void_p)
    for flags in (2, 4, 0x80000000, 3):
        assert f(fake, 1, one, off, br, flags, one, one, ix, one, None, None, None) == -1
    assert f(fake, 1, one, off, br, PHGR, one, one, ix, one, None, None, one) == -1   # desc_status without desc_off
    assert f(fake, 1, None, off, br, PHGR, one, one, ix, one, None, None, None) == -1


def test_phgr_kernels_stay_in_registers():
    from tools import resource_table
    with tempfile.TemporaryDirectory() as tmp:
        rows = {r["name"]: r for r in resource_table.unit("zg_shielded_phgr.hip", tmp) if "occ" in r}
    assert len(rows) == len(CEILINGS), sorted(rows)
    for part, (vgpr, scratch, lds) in CEILINGS.items():
        (name, r), = [(n, r) for n, r in rows.items() if part in n]
        assert r["vgpr"] <= vgpr and r["scratch"] <= scratch and r["lds"] <= lds, (name, r)
        assert r.get("vspill", 0) == 0 and r.get("sspill", 0) == 0 and r["occ"] >= 2, (name, r)


# ------------------------------------------------------------------ the collector, with a stand-in verifier
def test_collector_option():
    from zebra_amd.collector import Tx, verify_block
    calls = []

    def backend(txs, branch_ids, phgr=False):
        calls.append((len(txs), phgr))
        return P.run(txs, branch_ids, PHGR if phgr else 0)
    cs = {c[0]: c for c in C.cases() + C4.cases()}
    tx = lambda name, **kw: Tx(raw=cs[name][1], branch_id=cs[name][2], shielded=True, **kw)  # noqa: E731
    kw = dict(verify=lambda *a: [], shielded_verify=backend)
    ok = [tx("sap0"), tx("real0"), tx("js0"), tx("real4"), tx("v1")]
    assert verify_block(ok, shielded_phgr=True, **kw) is None and calls == [(5, True)]
    assert verify_block(ok + [tx("own_key")], shielded_phgr=True, **kw) == (5, ("InvalidJoinSplit", 0))
    assert verify_block(ok + [tx("proof_byte_1")], shielded_phgr=True, **kw) == (5, "JoinSplitSignature")
    assert verify_block([tx("real4", tree_errors=[None, "UnknownAnchor"])], shielded_phgr=True, **kw) == (0, "UnknownAnchor")
    assert verify_block([tx("own_key", tree_errors=["UnknownAnchor"])], shielded_phgr=True, **kw) == \
        (0, ("InvalidJoinSplit", 0))
    assert verify_block([tx("real0", js_nullifier_error="JoinSplitDeclared")], shielded_phgr=True, **kw) == \
        (0, "JoinSplitDeclared")
    # without the option nothing changes: the call carries no phgr argument and HOST raises
    n = len(calls)
    with pytest.raises(zg.ZgError):
        verify_block(ok, **kw)
    assert calls[n:] == [(5, False)]
    assert verify_block([tx("sap0"), tx("js0")], **kw) is None
