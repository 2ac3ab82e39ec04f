"""PHGR JoinSplit transactions from their bytes on the GPU (zg_shielded_verify_flags with
ZG_SHIELDED_PHGR): statuses, indices, details, hashes and the per-description classes against
tests/shielded_phgr_ref.py, exactly. The cases are those of tests/shielded_phgr_cases.py; the reference's PGHR13
verdicts are the recorded ones of tests/golden/phgr_txs.json."""
import os

import pytest

from tests import shielded_cases as C4
from tests import shielded_phgr_cases as C
from tests import shielded_phgr_ref as P
from tests import shielded_ref as S

pytestmark = pytest.mark.gpu

WHAT = ("tx_status", "status", "index", "detail", "hashes", "desc_status")


@pytest.fixture(scope="module")
def ctx():
    from zebra_amd import Context
    return Context(device=0, max_batch=64)


@pytest.fixture(scope="module")
def ctx64():
    """ZG_PGHR_CHUNK = 64, set the way tests/test_gpu_pghr13_edges.py sets its knobs: the PHGR rows of a window cross
    chunk boundaries; a chunk with a failure takes the per-proof path, the others the batch check"""
    from zebra_amd import Context
    old = os.environ.get("ZG_PGHR_CHUNK")
    os.environ["ZG_PGHR_CHUNK"] = "64"
    try:
        c = Context(device=0, max_batch=64)
    finally:
        if old is None:
            del os.environ["ZG_PGHR_CHUNK"]
        else:
            os.environ["ZG_PGHR_CHUNK"] = old
    yield c
    c.close()


def check(ctx, txs, branch_ids, names=None, phgr=True):
    got = ctx.shielded_verify(txs, branch_ids, phgr=phgr)
    want = P.run(txs, branch_ids, P.SHIELDED_PHGR if phgr else 0)
    for k, what in enumerate(WHAT):
        for t in range(len(txs)):
            assert got[k][t] == want[k][t], (what, t, names[t] if names else None, got[k][t], want[k][t])
    return got


def test_every_case_in_one_call(ctx):
    cs = C.cases()
    got = check(ctx, [c[1] for c in cs], [c[2] for c in cs], [c[0] for c in cs])
    assert set(got[1]) == {S.SHTX_OK, S.SHTX_JOINSPLIT_SIGNATURE, S.SHTX_INVALID_JOINSPLIT}
    assert {S.SHD_ED_PUBLIC_ENCODING, S.SHD_ED_SIGNATURE_ENCODING, S.SHD_ED_SIGNATURE, S.SHD_JOINSPLIT_ENCODING,
            P.SHD_JOINSPLIT_PGHR_PROOF} <= set(got[3])
    for i in range(5):   # the hash is the one the real signature verifies under
        assert got[1][i] == S.SHTX_OK and got[4][i] != S.ZERO


def test_interleaved_with_the_f17_cases(ctx):
    cs = C.interleaved_cases()
    got = check(ctx, [c[1] for c in cs], [c[2] for c in cs], [c[0] for c in cs])
    assert S.SHTX_HOST not in got[1] and set(range(8)) - {S.SHTX_HOST} <= set(got[1])


def test_without_the_flag_nothing_changes(ctx):
    cs = C.interleaved_cases()
    txs, br = [c[1] for c in cs], [c[2] for c in cs]
    before = ctx.stats()["pghr13_calls"]
    got = check(ctx, txs, br, [c[0] for c in cs], phgr=False)
    assert got == ctx.shielded_verify(txs, br) == ctx.shielded_verify(txs, br, flags=0)
    n = 0
    for t, c in enumerate(cs):
        if got[1][t] == S.SHTX_HOST:
            assert (got[2][t], got[3][t], got[4][t], got[5][t]) == (0, 0, S.ZERO, []), c[0]
            n += 1
    assert n == len(C.cases()) + 1 and ctx.stats()["pghr13_calls"] == before


def test_optional_outputs(ctx):
    cs = C.cases()[:8]
    txs, br = [c[1] for c in cs], [c[2] for c in cs]
    full = ctx.shielded_verify(txs, br, phgr=True)
    bare = ctx.shielded_verify(txs, br, want_hashes=False, want_desc=False, phgr=True)
    assert bare[:4] == full[:4] and bare[4] is None and bare[5] is None


def test_spliced_positions_across_chunks(ctx64):
    """130 copies of one description in one transaction, the bad one at 0, 63, 64 and last: 520 rows in chunks of 64"""
    pos = (0, 63, 64, 129)
    txs = [C.spliced(130, j) for j in pos]
    before = ctx64.stats()
    got = check(ctx64, txs, [0] * len(txs))
    for j, row in zip(pos, got[5]):
        assert row == [P.SHD_JOINSPLIT_PGHR_PROOF if i == j else 0 for i in range(130)]
    after = ctx64.stats()
    assert after["pghr13_calls"] == before["pghr13_calls"] + 1
    assert after["pghr13_batch_failures"] == before["pghr13_batch_failures"] + 1


@pytest.mark.parametrize("n_phgr", [1, 63, 64, 65, 130])
def test_mixed_windows(ctx64, n_phgr):
    """n PHGR descriptions beside 65 Groth16 descriptions, max_batch = 64 and chunks of 64; the first and the last
    PHGR description failing, as the first and the last Groth16 description do"""
    txs, br = C.mixed_window(n_phgr)
    got = check(ctx64, txs, br)
    pg = [row for raw, row in zip(txs, got[5]) if C.R.parse(raw)[1]["sigver"] != 2]
    v4 = [row for raw, row in zip(txs, got[5]) if C.R.parse(raw)[1]["sigver"] == 2]
    assert sum(len(r) for r in pg) == n_phgr and sum(len(r) for r in v4) == 65
    assert pg[0][0] == P.SHD_JOINSPLIT_PGHR_PROOF and pg[-1][-1] == P.SHD_JOINSPLIT_PGHR_PROOF
    assert sum(1 for r in pg for c in r if c) == min(n_phgr, 2)
    assert v4[0] == [S.SHD_VALUE_COMMITMENT_SMALL_ORDER] and v4[-1] == [S.SHD_PROOF_INVALID]


def test_phgr_only_window_and_the_counters(ctx64):
    """no Groth16 row at all; an all-valid window moves [8] by one and leaves [9]"""
    txs = C.phgr_window(70, fail_ends=False)
    before = ctx64.stats()
    got = check(ctx64, txs, [0] * len(txs))
    assert set(got[1]) == {S.SHTX_OK} and sum(len(r) for r in got[5]) == 70
    after = ctx64.stats()
    assert after["pghr13_calls"] == before["pghr13_calls"] + 1
    assert after["pghr13_batch_failures"] == before["pghr13_batch_failures"]
    assert after["batches"] == before["batches"]
    check(ctx64, C.phgr_window(70), [0] * len(C.phgr_window(70)))
    assert ctx64.stats()["pghr13_batch_failures"] == before["pghr13_batch_failures"] + 1


def test_v4_only_window_with_the_flag(ctx):
    txs, br = C4.window(65)
    before = ctx.stats()["pghr13_calls"]
    assert ctx.shielded_verify(txs, br, phgr=True) == ctx.shielded_verify(txs, br)
    assert ctx.stats()["pghr13_calls"] == before


@pytest.mark.parametrize("lead", [0, 1, 2, 3])
def test_every_alignment(ctx, lead):
    """the same window behind a malformed leading slice of 0..3 bytes: every field a lane reads starts at each
    residue mod 4"""
    cs = C.interleaved_cases()
    txs, br = [bytes(lead)] + [c[1] for c in cs], [0] + [c[2] for c in cs]
    got = check(ctx, txs, br)
    assert got[1][0] == S.SHTX_TX_MALFORMED


def test_nothing_to_launch_and_the_key_rule(ctx):
    cs = {c[0]: c for c in C4.cases()}
    pick = [cs[k] for k in ("v1", "v3_none", "truncated", "noncanonical")]
    before = ctx.stats()["pghr13_calls"]
    got = check(ctx, [c[1] for c in pick], [c[2] for c in pick])
    assert got[1] == [S.SHTX_NONE, S.SHTX_NONE, S.SHTX_TX_MALFORMED, S.SHTX_TX_NONCANONICAL]
    assert ctx.stats()["pghr13_calls"] == before
    assert ctx.shielded_verify([], [], phgr=True) == ([], [], [], [], [], [])
    from zebra_amd import Context, zg
    bare = Context(device=0, max_batch=64, load_builtin=False)
    with pytest.raises(zg.ZgError) as e:   # the three Groth16 keys, whatever the window holds
        bare.shielded_verify([C.real()[0]], [0], phgr=True)
    assert e.value.code == -3
    with pytest.raises(zg.ZgError) as e:
        ctx.shielded_verify([C.real()[0]], [0], flags=2)
    assert e.value.code == -1
    bare.close()


def test_agrees_with_the_four_call_path(ctx):
    """zg_sighash, zg_prep_batch with ZG_PREP_KIND_JOINSPLIT_BN, zg_pghr13_verify and zg_ed25519_verify over
    host-sliced fields, folded here in the reference's order, transaction by transaction"""
    from zebra_amd import zg
    cs = C.cases()
    txs, br = [c[1] for c in cs], [c[2] for c in cs]
    got = ctx.shielded_verify(txs, br, phgr=True)
    ts, hashes, hst = ctx.sighash(txs, br, [(t, None, b"", 0, 1) for t in range(len(txs))])
    assert set(ts) == {0} and set(hst) == {0} and hashes == got[4]
    parsed = [C.parsed(raw) for raw in txs]
    fields, proofs, owner = [], [], []
    for t, p in enumerate(parsed):
        for d in p["joinsplits"]:
            fields.append(zg.prep_fields(zg.PREP_KIND_JOINSPLIT_BN, d[16:48], d[208:240], [d[48:80], d[80:112]],
                                         [d[240:272], d[272:304]], [d[112:144], d[144:176]],
                                         int.from_bytes(d[0:8], "little"), int.from_bytes(d[8:16], "little"),
                                         p["js_pubkey"]))
            proofs.append(d[304:600])
            owner.append(t)
    n = len(proofs)
    rows, codes = ctx.prep_batch(bytes([zg.PREP_KIND_JOINSPLIT_BN]) * n, b"".join(fields))
    assert set(codes) == {0}
    pst = ctx.pghr13_verify(b"".join(proofs), rows, bytes([9]) * n)
    ed = ctx.ed25519_verify([p["js_pubkey"] for p in parsed], [p["js_sig"] for p in parsed], hashes)
    for t, (name, _, _) in enumerate(cs):
        js = [P.desc_class(s) for s, o in zip(pst, owner) if o == t]
        first = (S.SHTX_OK, 0, 0)
        if ed[t]:
            first = (S.SHTX_JOINSPLIT_SIGNATURE, 0, S.SHD_ED_PUBLIC_ENCODING - 1 + ed[t])
        for i, c in enumerate(js):
            if c and first[0] == S.SHTX_OK:
                first = (S.SHTX_INVALID_JOINSPLIT, i, c)
        assert (got[1][t], got[2][t], got[3][t], got[5][t]) == first + (js,), name


def test_collector_against_the_existing_phgr_path(ctx):
    """verify_block with shielded_phgr over marked transactions against the host-sliced PHGR path of the collector,
    on block 522's transactions mixed with the Groth16 transactions, in the precedence steps of
    tests/test_collector.py::_pghr_cases"""
    from zebra_amd import collector
    r4 = C4.real()
    groth = [r4[k] for k in ("sap0", "js0", "sap1")]
    bad1 = [x[1] for x in C.cases() if x[0] == "own_key_proof_byte_1"][0]
    enc0 = [x[1] for x in C.cases() if x[0].startswith("own_key_encoding_0_")][0]
    windows = [groth + list(C.real()),
               groth + list(C.real()[:4]) + [[x[1] for x in C.cases() if x[0] == "own_key"][0]],
               groth + list(C.real()[:4]) + [bad1],
               groth + list(C.real()[:4]) + [enc0],
               groth + [C.build(C.own_key(C.parsed(C.real()[1])))] + list(C.real()[2:4]) + [enc0],
               [C4.cases()[[c[0] for c in C4.cases()].index("spend_own_key")][1]] + list(C.real()[:4]) + [enc0]]
    for k, w in enumerate(windows):
        for tree in (None, "UnknownAnchor"):
            old = [C4.collector_tx(raw) if C.R.parse(raw)[1]["sigver"] == 2 else C.collector_tx(raw) for raw in w]
            new = [collector.Tx(raw=raw, branch_id=C.branch(raw), shielded=True) for raw in w]
            for a, b in zip(old, new):   # the root of every first description fails: on the description in the
                if tree and a.joinsplits:  # host-sliced view, in tree_errors in the marked one
                    a.joinsplits[0].tree_error = tree
                    b.tree_errors = [tree]
            want = collector.verify_block(old, ctx=ctx)
            assert collector.verify_block(new, ctx=ctx, shielded_phgr=True) == want, (k, tree, want)
            if k == 0 and tree is None:
                assert want is None
    with pytest.raises(collector.zg.ZgError):
        collector.verify_block([collector.Tx(raw=C.real()[0], branch_id=0, shielded=True)], ctx=ctx)
